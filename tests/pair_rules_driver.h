// A scalar host driver of bwa-meme_amd/csrc/meme_pair_rules.h: mem_pair for the pairs of a batch, one after the other.  tests/test_pair_rules_model.py compiles
// it with g++ into a shared object; scripts/pair_rules_main.cpp wraps it in a program of its own (for a sanitizer build).  Nothing here decides a result: the
// order of the keys is klib's introsort (meme_ksort.h) over a column of indices with the header's less-than, the candidates are every k < i the header's
// predicate admits (no y[], no skip on `which`: what the kernels do -- a walk towards smaller k that ends beyond the reach of every live orientation, or, with
// t_pair_exhaustive(1), over every k < i), the penalties are a table the host's libm fills as the stage's host part does,
// and the two largest candidates and the count behind them come from the header's top-two.
#pragma once
#include <stdint.h>
#include <vector>

#include "meme_pair_rules.h"

namespace pair_driver {

struct Stack {                               // ks_introsort's stack
    std::vector<int> v;
    void push(int l, int r, int d) { v.push_back(l); v.push_back(r); v.push_back(d); }
    bool pop(int& l, int& r, int& d) { if (v.empty()) return false; d = v.back(); v.pop_back(); r = v.back(); v.pop_back(); l = v.back(); v.pop_back(); return true; }
};
struct Before {
    const PairKey* a;
    bool operator()(int x, int y) const { return pair_lt(a[x], a[y]); }
};
// the orientations and the penalty table of a call; false: an orientation spans more distances than the table holds
inline bool table(const meme_pair_pes* pes, int a, PairDirs* D, std::vector<double>* tab) {
    tab->clear();
    for (int d = 0; d < 4; ++d) {
        D->low[d] = pes[d].low; D->high[d] = pes[d].high; D->failed[d] = pes[d].failed ? 1 : 0; D->tab_off[d] = (int64_t)tab->size();
        if (D->failed[d] || pes[d].high < pes[d].low) continue;
        if ((int64_t)pes[d].high - pes[d].low + 1 > PAIR_TABLE_MAX) return false;
        for (int64_t dist = pes[d].low; dist <= pes[d].high; ++dist) tab->push_back(pair_penalty(dist, pes[d].avg, pes[d].std, a));
    }
    tab->push_back(0.);
    return true;
}

static bool exhaustive = false;               // true: every k < i is put to the predicate, none skipped as beyond the reach

}  // namespace pair_driver

extern "C" void t_pair_exhaustive(int on) { pair_driver::exhaustive = on != 0; }

// per pair (reads 2p, 2p + 1): score, sub, n_sub, n_cand, status; z two per pair.  -> 0, or -1 where the table cannot be built
extern "C" int t_pair(const meme_alnreg* regs, const int64_t* reg_off, const int32_t* n_pri, int64_t nreads, const meme_contig* contigs, int32_t n_contigs, int64_t l_pac,
                      const meme_pair_pes* pes, int64_t id_base, const meme_pair_opt* opt, int32_t* score, int32_t* sub, int32_t* n_sub, int32_t* n_cand, int32_t* z, uint8_t* status) {
    using namespace pair_driver;
    PairDirs D;
    std::vector<double> tab;
    if (!table(pes, opt->a, &D, &tab)) return -1;
    const int tmp = pair_score_distance(*opt);
    std::vector<PairKey> v, s;
    std::vector<int> ord;
    for (int64_t p = 0; p < nreads / 2; ++p) {
        score[p] = sub[p] = n_sub[p] = n_cand[p] = 0; z[2 * p] = z[2 * p + 1] = -1; status[p] = 0;
        if (n_pri[2 * p] <= 0 || n_pri[2 * p + 1] <= 0) continue;
        v.clear();
        bool ok = true;
        for (int r = 0; r < 2; ++r)
            for (int i = 0; i < n_pri[2 * p + r]; ++i) {
                const meme_alnreg& R = regs[reg_off[2 * p + r] + i];
                if (!pair_record_ok(R.rid, R.score, n_contigs)) { ok = false; continue; }
                v.push_back(pair_key(R.rb, R.rid, R.score, i, r, l_pac, contigs[R.rid].offset));
            }
        if (!ok) { status[p] = 1; continue; }
        const int m = (int)v.size();
        ord.resize((size_t)m);
        for (int k = 0; k < m; ++k) ord[(size_t)k] = k;
        Stack st;
        ks_introsort(KsPtr<int>{ord.data()}, m, Before{v.data()}, st);
        s.resize((size_t)m);
        for (int k = 0; k < m; ++k) s[(size_t)k] = v[(size_t)ord[(size_t)k]];
        const uint64_t idx = pair_idx((uint64_t)id_base + (uint64_t)p);
        const int64_t reach = pair_reach(D);
        PairTop top = pair_top_none();
        for (int pass = 0; pass < 2; ++pass)                                       // the candidates twice, as the wavefront tier enumerates them: the top two, then n_sub
            for (int i = 0; i < m; ++i)
                for (int k = i - 1; k >= 0 && (exhaustive || !pair_beyond(s[(size_t)i], s[(size_t)k], reach)); --k) {
                    int64_t dist;
                    const int dir = pair_candidate(s[(size_t)i], s[(size_t)k], D, &dist);
                    if (dir < 0) continue;
                    const double T = tab[(size_t)(pair_pick64(D.tab_off, dir) + (dist - pair_pick(D.low, dir)))];
                    const PairKey c = pair_cand_key(pair_q(pair_key_score(s[(size_t)i]), pair_key_score(s[(size_t)k]), T), k, i, idx);
                    if (pass == 0) top = pair_top_push(top, c);
                    else n_sub[p] += pair_in_n_sub(c, top, tmp);
                }
        score[p] = pair_top_score(top); sub[p] = pair_top_sub(top); n_cand[p] = top.n;
        if (top.n) {
            const PairKey first = s[(size_t)(top.best.y >> 32)], second = s[(size_t)(top.best.y & 0xffffffffu)];
            z[2 * p + pair_key_end(first)] = pair_key_index(first);
            z[2 * p + pair_key_end(second)] = pair_key_index(second);
        }
    }
    return 0;
}
