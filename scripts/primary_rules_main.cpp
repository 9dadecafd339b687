// The sequential driver of bwa-meme_amd/csrc/meme_primary_rules.h (tests/primary_rules_driver.h) over a dumped workload, as a program of its own -- for a sanitizer
// build of the rules both tiers of meme_primary.hip call:
//   python scripts/primary_rules_dump.py /tmp/primary.bin
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Ibwa-meme_amd/csrc -Itests scripts/primary_rules_main.cpp -o /tmp/primary_rules_main
//   /tmp/primary_rules_main /tmp/primary.bin
// The dump (primary_rules_dump.py): four int64 -- reads, records, the id of read 0, the read whose qualities need a logarithm beyond the table -- then reg_off, the records,
// and what is expected: the records in their final order, n_pri per read, the quality per record.  The workload runs with the default options and again with primary5.
// Exit status 0: every byte the functions decide equals the expectation.
#include <stdio.h>
#include <string.h>

#include "primary_rules_driver.h"

template <class T> static bool take(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s DUMP\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int64_t h[4];
    if (fread(h, 8, 4, f) != 4) { fprintf(stderr, "short header\n"); return 2; }
    const int64_t nreads = h[0], nregs = h[1], id_base = h[2], status_read = h[3];
    std::vector<int64_t> reg_off;
    std::vector<meme_alnreg> regs, want;
    std::vector<int32_t> want_n_pri;
    std::vector<uint8_t> want_mapq;
    if (!take(f, reg_off, nreads + 1) || !take(f, regs, nregs) || !take(f, want, nregs) || !take(f, want_n_pri, nreads) || !take(f, want_mapq, nregs)) { fprintf(stderr, "short dump\n"); return 2; }
    fclose(f);
    meme_primary_opt o = {1, 4, 6, 1, 6, 1, 19, 30, 0.5f, 50.f, 3, 0};
    std::vector<meme_alnreg> out(nregs + 1);
    std::vector<int32_t> n_pri(nreads + 1);
    std::vector<uint8_t> mapq(nregs + 1), status(nreads + 1);
    t_primary(regs.data(), reg_off.data(), nreads, id_base, &o, out.data(), n_pri.data(), mapq.data(), status.data());
    int64_t bad = 0;
    for (int64_t r = 0; r < nreads; ++r) {
        bad += n_pri[r] != want_n_pri[r] || status[r] != (r == status_read ? 1 : 0);
        for (int64_t k = reg_off[r]; k < reg_off[r + 1]; ++k) {
            const meme_alnreg &a = out[k], &b = want[k];
            bad += a.rb != b.rb || a.re != b.re || a.qb != b.qb || a.qe != b.qe || a.rid != b.rid || a.c != b.c || a.score != b.score || a.truesc != b.truesc || a.sub != b.sub || a.alt_sc != b.alt_sc ||
                   a.csub != b.csub || a.sub_n != b.sub_n || a.w != b.w || a.seedcov != b.seedcov || a.secondary != b.secondary || a.secondary_all != b.secondary_all || a.seedlen0 != b.seedlen0 ||
                   a.n_comp_is_alt != b.n_comp_is_alt || memcmp(&a.frac_rep, &b.frac_rep, 4) || a.hash != b.hash || a.flg != b.flg || (r != status_read && mapq[k] != want_mapq[k]);
        }
    }
    const int64_t orders = t_primary_orders();
    // primary5: no expectation in the dump; every read keeps its records (the sum of c, which no function writes) and its first record is no secondary
    o.primary5 = 1;
    t_primary(regs.data(), reg_off.data(), nreads, id_base, &o, out.data(), n_pri.data(), mapq.data(), status.data());
    for (int64_t r = 0; r < nreads; ++r) {
        uint64_t s_in = 0, s_out = 0;
        for (int64_t k = reg_off[r]; k < reg_off[r + 1]; ++k) { s_in += regs[k].c; s_out += out[k].c; }
        bad += s_in != s_out || (reg_off[r + 1] > reg_off[r] && out[reg_off[r]].secondary >= 0);
    }
    printf("reads %lld, records %lld, %lld orders taken, %lld differences\n", (long long)nreads, (long long)nregs, (long long)orders, (long long)bad);
    return bad ? 1 : 0;
}
