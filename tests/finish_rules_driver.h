// A scalar host driver of bwa-meme_amd/csrc/meme_finish_rules.h: finish_read over the reads of a batch with the header's own scalar patch score.
// tests/test_finish_rules_model.py compiles it with g++ into a shared object; scripts/finish_rules_main.cpp wraps it in a program of its own (for a
// sanitizer build).  Nothing here decides a result: the records are laid out as columns, handed to the driver and read back.
#pragma once
#include <stdint.h>
#include <vector>

#include "meme_finish_rules.h"

// -> records left; counters[0] += patch alignments asked for, counters[1] += merges
extern "C" int64_t t_finish(const meme_alnreg* regs, const int64_t* reg_off, int64_t nreads, const uint8_t* reads, const int64_t* read_off, const uint8_t* text, int64_t l_pac,
                            const unsigned char* alt, int n_contigs, const meme_finish_opt* o, meme_alnreg* out, int64_t* off_out, uint8_t* ums, uint8_t* status, int64_t* counters) {
    std::vector<int> c, stack(3 * FIN_STACK), h(FIN_MAX_QLEN + 2), e(FIN_MAX_QLEN + 2);
    std::vector<long long> l;
    int64_t total = 0;
    off_out[0] = 0;
    for (int64_t r = 0; r < nreads; ++r) {
        const int64_t base = reg_off[r];
        const int n_in = (int)(reg_off[r + 1] - base), cap = n_in > 0 ? n_in : 1;
        c.assign((size_t)FIN_INTS * cap, 0);
        l.assign((size_t)FIN_LONGS * cap, 0);
        const FinCols s = {c.data(), l.data(), cap};
        for (int k = 0; k < n_in; ++k) {
            const meme_alnreg& R = regs[base + k];
            s.setl(FIN_RB, k, R.rb); s.setl(FIN_RE, k, R.re);
            s.seti(FIN_QB, k, R.qb); s.seti(FIN_QE, k, R.qe); s.seti(FIN_RID, k, R.rid); s.seti(FIN_SCORE, k, R.score); s.seti(FIN_TRUESC, k, R.truesc); s.seti(FIN_SUB, k, R.sub);
            s.seti(FIN_CSUB, k, R.csub); s.seti(FIN_SEEDCOV, k, R.seedcov); s.seti(FIN_W, k, R.w); s.seti(FIN_NCOMP, k, R.n_comp_is_alt & 0x3fffffff);
        }
        const uint8_t* rd = reads + read_off[r];
        const int read_len = (int)(read_off[r + 1] - read_off[r]);
        FinStack st = {stack.data(), 0};
        FinRead res;
        const int m = finish_read(s, n_in, read_len, l_pac, *o, [&](const FinPose& P, int64_t rb, int qb) -> int {
            return fin_patch_score(P, rb, qb, [&](int64_t p) -> int { return text[p]; }, [&](int j) -> int { return rd[j]; }, *o, h.data(), e.data());
        }, st, &res);
        for (int k = 0; k < m; ++k) {
            const int x = s.geti(FIN_ORD, k);
            meme_alnreg R = regs[base + x];
            R.rb = s.getl(FIN_RB, x); R.re = s.getl(FIN_RE, x);
            R.qb = s.geti(FIN_QB, x); R.qe = s.geti(FIN_QE, x); R.score = s.geti(FIN_SCORE, x); R.truesc = s.geti(FIN_TRUESC, x); R.sub = s.geti(FIN_SUB, x); R.csub = s.geti(FIN_CSUB, x);
            R.seedcov = s.geti(FIN_SEEDCOV, x); R.w = s.geti(FIN_W, x);
            R.n_comp_is_alt = fin_word(R.n_comp_is_alt, s.geti(FIN_NCOMP, x), R.rid, alt, n_contigs);
            out[total + k] = R;
        }
        total += m;
        off_out[r + 1] = total;
        ums[r] = (uint8_t)res.use_mate_sort;
        status[r] = (uint8_t)res.status;
        counters[0] += res.n_jobs;
        counters[1] += res.n_merged;
    }
    return total;
}

// the score bwa_gen_cigar2 returns for query span [qb, qe) of a read against [rb, re) of the fwd + rc text with the band argument w_; *ok = 0: a call the function rejects
extern "C" int t_patch_score(const uint8_t* text, int64_t l_pac, const uint8_t* read, int read_len, int qb, int qe, int64_t rb, int64_t re, int w_, const meme_finish_opt* o, int* ok) {
    const FinPose P = fin_pose(l_pac, qb, qe, read_len, rb, re, w_, *o);
    *ok = P.ok;
    if (!P.ok) return 0;
    std::vector<int> h(FIN_MAX_QLEN + 2), e(FIN_MAX_QLEN + 2);
    return fin_patch_score(P, rb, qb, [&](int64_t p) -> int { return text[p]; }, [&](int j) -> int { return read[j]; }, *o, h.data(), e.data());
}
