// The sequential driver of bwa-meme_amd/csrc/meme_decide_rules.h (tests/decide_rules_driver.h) over a dumped workload, as a program of its own -- for a sanitizer
// build of the rules meme_decide.hip's kernel calls (tests/test_decide_rules_model.py builds and runs it this way):
//   python scripts/decide_rules_dump.py /tmp/decide.bin
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Ibwa-meme_amd/csrc -Itests scripts/decide_rules_main.cpp -o /tmp/decide_rules_main
//   /tmp/decide_rules_main /tmp/decide.bin
// The dump (tests/decide_cases.py: dump): int64 batches; per batch int64 reads, records; the options; the four orientations; reg_off, n_pri, the pair stage's score, sub,
// n_sub, z and status, the records; and what is expected: path, sel, q_se, q_pe, flag, alt, status and the records behind the decision.
// Exit status 0: every value and every byte of every record equals the expectation.
#include <stdio.h>
#include <string.h>

#include "decide_rules_driver.h"

template <class T> static bool take(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, f) == n; }
template <class T> static long long differ(const std::vector<T>& a, const std::vector<T>& b, size_t n) { long long d = 0; for (size_t k = 0; k < n; ++k) d += a[k] != b[k]; return d; }

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s DUMP\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int64_t nbatches = 0;
    if (fread(&nbatches, 8, 1, f) != 1) { fprintf(stderr, "short header\n"); return 2; }
    long long bad = 0, pairs = 0, records = 0;
    for (int64_t b = 0; b < nbatches; ++b) {
        int64_t h[2];
        meme_decide_opt o;
        meme_pair_pes pes[4];
        if (fread(h, 8, 2, f) != 2 || fread(&o, sizeof(o), 1, f) != 1 || fread(pes, sizeof(meme_pair_pes), 4, f) != 4) { fprintf(stderr, "short batch header\n"); return 2; }
        const size_t nreads = (size_t)h[0], nregs = (size_t)h[1], np = nreads / 2;
        std::vector<int64_t> reg_off;
        std::vector<int32_t> n_pri, score, sub, n_sub, z, w_path, w_sel, w_q_se, w_q_pe, w_flag, w_alt;
        std::vector<uint8_t> pair_status, w_status;
        std::vector<meme_alnreg> regs, w_regs;
        if (!take(f, reg_off, nreads + 1) || !take(f, n_pri, nreads) || !take(f, score, np) || !take(f, sub, np) || !take(f, n_sub, np) || !take(f, z, 2 * np) || !take(f, pair_status, np) ||
            !take(f, regs, nregs) || !take(f, w_path, np) || !take(f, w_sel, 2 * np) || !take(f, w_q_se, 2 * np) || !take(f, w_q_pe, np) || !take(f, w_flag, np) || !take(f, w_alt, 2 * np) ||
            !take(f, w_status, np) || !take(f, w_regs, nregs)) {
            fprintf(stderr, "short dump\n");
            return 2;
        }
        std::vector<int32_t> path(np), sel(2 * np), q_se(2 * np), q_pe(np), flag(np), alt(2 * np);
        std::vector<uint8_t> status(np);
        if (t_decide(regs.data(), reg_off.data(), n_pri.data(), (int64_t)nreads, score.data(), sub.data(), n_sub.data(), z.data(), pair_status.data(), 300000, pes, &o, path.data(), sel.data(),
                     q_se.data(), q_pe.data(), flag.data(), alt.data(), status.data())) { fprintf(stderr, "batch %lld refused\n", (long long)b); return 2; }
        bad += differ(path, w_path, np) + differ(sel, w_sel, 2 * np) + differ(q_se, w_q_se, 2 * np) + differ(q_pe, w_q_pe, np) + differ(flag, w_flag, np) + differ(alt, w_alt, 2 * np) +
               differ(status, w_status, np);
        bad += nregs && memcmp(regs.data(), w_regs.data(), nregs * sizeof(meme_alnreg)) != 0;
        pairs += (long long)np; records += (long long)nregs;
    }
    fclose(f);
    printf("batches %lld, pairs %lld, records %lld, %lld differences\n", (long long)nbatches, pairs, records, bad);
    return bad ? 1 : 0;
}
