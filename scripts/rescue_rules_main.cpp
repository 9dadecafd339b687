// The sequential driver of bwa-meme_amd/csrc/meme_rescue_rules.h (tests/rescue_rules_driver.h) over a dumped workload, as a program of its own -- for a sanitizer
// build of the rules meme_rescue.hip's kernels call (tests/test_rescue_rules_model.py builds and runs it this way):
//   PYTHONPATH=bwa-meme_amd:tests python -c "import rescue_cases; rescue_cases.dump('/tmp/rescue.bin')"
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Ibwa-meme_amd/csrc -Itests scripts/rescue_rules_main.cpp -o /tmp/rescue_rules_main
//   /tmp/rescue_rules_main /tmp/rescue.bin
// The dump (tests/rescue_cases.py: dump): int64 batches; per batch int64 reads, records, gar entries, worker batches, jobs, records expected; the options; the four
// orientations; the contigs (int64 count, then meme_contig); reg_off, use_mate_sort, read_len, gar, gar_off, job_off, res, the records; and what is expected: reg_off,
// status, four counters and the records behind the stage.
// Exit status 0: every value and every byte of every record equals the expectation.
#include <stdio.h>
#include <string.h>

#include "rescue_rules_driver.h"

template <class T> static bool take(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, f) == n; }
template <class T> static long long differ(const std::vector<T>& a, const std::vector<T>& b, size_t n) { long long d = 0; for (size_t k = 0; k < n; ++k) d += a[k] != b[k]; return d; }

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s DUMP\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int64_t nbatches = 0;
    if (fread(&nbatches, 8, 1, f) != 1) { fprintf(stderr, "short header\n"); return 2; }
    long long bad = 0, reads = 0, records = 0;
    for (int64_t b = 0; b < nbatches; ++b) {
        int64_t h[6], nc = 0;
        meme_rescue_opt o;
        meme_pestat pes[4];
        if (fread(h, 8, 6, f) != 6 || fread(&o, sizeof(o), 1, f) != 1 || fread(pes, sizeof(meme_pestat), 4, f) != 4 || fread(&nc, 8, 1, f) != 1) { fprintf(stderr, "short batch header\n"); return 2; }
        const size_t nreads = (size_t)h[0], nregs = (size_t)h[1], ngar = (size_t)h[2], nb = (size_t)h[3], nj = (size_t)h[4], nwant = (size_t)h[5];
        std::vector<meme_contig> contigs;
        std::vector<int64_t> reg_off, gar_off, job_off, w_off, w_ctr;
        std::vector<uint8_t> ums, w_status;
        std::vector<int32_t> rlen, gar;
        std::vector<meme_kswr> res;
        std::vector<meme_alnreg> regs, w_regs;
        if (!take(f, contigs, (size_t)nc) || !take(f, reg_off, nreads + 1) || !take(f, ums, nreads) || !take(f, rlen, nreads) || !take(f, gar, ngar) || !take(f, gar_off, nb + 1) ||
            !take(f, job_off, nb + 1) || !take(f, res, nj) || !take(f, regs, nregs) || !take(f, w_off, nreads + 1) || !take(f, w_status, nreads) || !take(f, w_ctr, 4) || !take(f, w_regs, nwant)) {
            fprintf(stderr, "short dump\n");
            return 2;
        }
        std::vector<meme_alnreg> out(nregs + nj + 1);
        std::vector<int64_t> off(nreads + 1), ctr(4);
        std::vector<uint8_t> status(nreads + 1);
        if (t_rescue(regs.data(), reg_off.data(), ums.data(), rlen.data(), (int64_t)nreads, gar.data(), gar_off.data(), job_off.data(), (int64_t)nb, res.data(), (int64_t)nj, pes, contigs.data(),
                     (int32_t)nc, 300000, &o, out.data(), off.data(), status.data(), ctr.data())) { fprintf(stderr, "batch %lld refused\n", (long long)b); return 2; }
        bad += differ(off, w_off, nreads + 1) + differ(status, w_status, nreads) + differ(ctr, w_ctr, 4);
        bad += (size_t)off[nreads] != nwant || (nwant && memcmp(out.data(), w_regs.data(), nwant * sizeof(meme_alnreg)) != 0);
        reads += (long long)nreads; records += (long long)nwant;
    }
    fclose(f);
    printf("batches %lld, reads %lld, records %lld, %lld differences\n", (long long)nbatches, reads, records, bad);
    return bad ? 1 : 0;
}
