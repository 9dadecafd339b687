// The sequential driver of bwa-meme_amd/csrc/meme_pair_rules.h (tests/pair_rules_driver.h) over a dumped workload, as a program of its own -- for a sanitizer
// build of the rules both tiers of meme_pair.hip call (tests/test_pair_rules_model.py builds and runs it this way):
//   python scripts/pair_rules_dump.py /tmp/pair.bin
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Ibwa-meme_amd/csrc -Itests scripts/pair_rules_main.cpp -o /tmp/pair_rules_main
//   /tmp/pair_rules_main /tmp/pair.bin
// The dump (tests/pair_cases.py: dump): int64 batches; per batch int64 reads, records, the id of pair 0; the four orientations; reg_off, n_pri, the records; and what is
// expected: score, sub, n_sub and z of every pair.  Every batch runs with the default options, once with the walk stopped at the reach and once over every k < i.
// Exit status 0: every value equals the expectation and both walks agree on n_cand.
#include <stdio.h>
#include <string.h>

#include "pair_rules_driver.h"

template <class T> static bool take(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s DUMP\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int64_t nbatches = 0;
    if (fread(&nbatches, 8, 1, f) != 1) { fprintf(stderr, "short header\n"); return 2; }
    const meme_contig contigs[3] = {{0, 100000, 0}, {100000, 100000, 0}, {200000, 100000, 1}};      // the fixture genome's
    const meme_pair_opt o = {1, 4, 6, 1, 6, 1};
    int64_t bad = 0, pairs = 0, cands = 0;
    for (int64_t b = 0; b < nbatches; ++b) {
        int64_t h[3];
        meme_pair_pes pes[4];
        if (fread(h, 8, 3, f) != 3 || fread(pes, sizeof(meme_pair_pes), 4, f) != 4) { fprintf(stderr, "short batch header\n"); return 2; }
        const int64_t nreads = h[0], nregs = h[1], id_base = h[2], np = nreads / 2;
        std::vector<int64_t> reg_off;
        std::vector<int32_t> n_pri, w_score, w_sub, w_n_sub, w_z;
        std::vector<meme_alnreg> regs;
        if (!take(f, reg_off, nreads + 1) || !take(f, n_pri, nreads) || !take(f, regs, nregs) || !take(f, w_score, np) || !take(f, w_sub, np) || !take(f, w_n_sub, np) || !take(f, w_z, 2 * np)) {
            fprintf(stderr, "short dump\n");
            return 2;
        }
        std::vector<int32_t> score[2], sub[2], n_sub[2], n_cand[2], z[2];
        std::vector<uint8_t> status[2];
        for (int e = 0; e < 2; ++e) {
            score[e].resize(np + 1); sub[e].resize(np + 1); n_sub[e].resize(np + 1); n_cand[e].resize(np + 1); z[e].resize(2 * np + 1); status[e].resize(np + 1);
            t_pair_exhaustive(e);
            if (t_pair(regs.data(), reg_off.data(), n_pri.data(), nreads, contigs, 3, 300000, pes, id_base, &o, score[e].data(), sub[e].data(), n_sub[e].data(), n_cand[e].data(), z[e].data(),
                       status[e].data())) { fprintf(stderr, "batch %lld refused\n", (long long)b); return 2; }
            for (int64_t p = 0; p < np; ++p)
                bad += score[e][p] != w_score[p] || sub[e][p] != w_sub[p] || n_sub[e][p] != w_n_sub[p] || z[e][2 * p] != w_z[2 * p] || z[e][2 * p + 1] != w_z[2 * p + 1] || status[e][p] != 0 ||
                       n_cand[e][p] != n_cand[0][p];
        }
        for (int64_t p = 0; p < np; ++p) cands += n_cand[0][p];
        pairs += np;
    }
    fclose(f);
    printf("batches %lld, pairs %lld, %lld candidates, %lld differences\n", (long long)nbatches, (long long)pairs, (long long)cands, (long long)bad);
    return bad ? 1 : 0;
}
