// What the record stages (record finishing, meme_finish.hip; primary marking, meme_primary.hip; pair scoring, meme_pair.hip) share of their plumbing: an
// alignment record in registers, a read's span of the record array, the argument checks of their host and device forms, the steps of a host form around its
// launch (upload, reserve, download, timing) and the clamps of their tuning keys.  Nothing here decides a result.
#pragma once
#include <limits.h>
#include <stddef.h>
#include <initializer_list>

#include "meme_common.h"

// A record in registers: seven 16-byte words (a record is 112 bytes and the record arrays are 16-byte aligned), the fields the stages touch by position.
struct RegWords {
    uint4 q0, q1, q2, q3, q4, q5, q6;
    __device__ __forceinline__ i64 rb() const { return (i64)((u64)q0.x | ((u64)q0.y << 32)); }
    __device__ __forceinline__ i64 re() const { return (i64)((u64)q0.z | ((u64)q0.w << 32)); }
    __device__ __forceinline__ int qb() const { return (int)q1.x; }
    __device__ __forceinline__ int qe() const { return (int)q1.y; }
    __device__ __forceinline__ int rid() const { return (int)q1.z; }
    __device__ __forceinline__ int score() const { return (int)q2.z; }
    __device__ __forceinline__ int sub() const { return (int)q3.x; }
    __device__ __forceinline__ int alt_sc() const { return (int)q3.y; }
    __device__ __forceinline__ int csub() const { return (int)q3.z; }
    __device__ __forceinline__ int sub_n() const { return (int)q3.w; }
    __device__ __forceinline__ int secondary() const { return (int)q4.z; }
    __device__ __forceinline__ int word() const { return (int)q5.y; }                            // n_comp:30, is_alt:2
    __device__ __forceinline__ int is_alt() const { return (int)q5.y >> 30; }
    __device__ __forceinline__ float frac_rep() const { return __uint_as_float(q5.z); }
    __device__ __forceinline__ void set_word(int v) { q5.y = (uint32_t)v; }
    __device__ __forceinline__ void set_span(i64 rb, i64 re, int qb, int qe) {
        q0.x = (uint32_t)(u64)rb; q0.y = (uint32_t)((u64)rb >> 32); q0.z = (uint32_t)(u64)re; q0.w = (uint32_t)((u64)re >> 32); q1.x = (uint32_t)qb; q1.y = (uint32_t)qe;
    }
    __device__ __forceinline__ void set_scores(int score, int truesc, int sub, int csub, int w, int seedcov) {
        q2.z = (uint32_t)score; q2.w = (uint32_t)truesc; q3.x = (uint32_t)sub; q3.z = (uint32_t)csub; q4.x = (uint32_t)w; q4.y = (uint32_t)seedcov;
    }
    __device__ __forceinline__ void set_marks(int sub, int alt_sc, int sub_n, int secondary, int secondary_all) { q3.x = (uint32_t)sub; q3.y = (uint32_t)alt_sc; q3.w = (uint32_t)sub_n; q4.z = (uint32_t)secondary; q4.w = (uint32_t)secondary_all; }
    __device__ __forceinline__ void set_secondary_all(int v) { q4.w = (uint32_t)v; }
    __device__ __forceinline__ void set_hash(u64 h) { q6.x = (uint32_t)h; q6.y = (uint32_t)(h >> 32); }
};
static_assert(sizeof(meme_alnreg) == 112 && offsetof(meme_alnreg, rb) == 0 && offsetof(meme_alnreg, re) == 8 && offsetof(meme_alnreg, qb) == 16 && offsetof(meme_alnreg, qe) == 20 &&
              offsetof(meme_alnreg, rid) == 24 && offsetof(meme_alnreg, score) == 40 && offsetof(meme_alnreg, truesc) == 44 && offsetof(meme_alnreg, sub) == 48 &&
              offsetof(meme_alnreg, alt_sc) == 52 && offsetof(meme_alnreg, csub) == 56 && offsetof(meme_alnreg, sub_n) == 60 && offsetof(meme_alnreg, w) == 64 &&
              offsetof(meme_alnreg, seedcov) == 68 && offsetof(meme_alnreg, secondary) == 72 && offsetof(meme_alnreg, secondary_all) == 76 && offsetof(meme_alnreg, n_comp_is_alt) == 84 &&
              offsetof(meme_alnreg, frac_rep) == 88 && offsetof(meme_alnreg, hash) == 96, "RegWords names meme_alnreg's fields by position");
__device__ __forceinline__ RegWords reg_load(const meme_alnreg* p) { const uint4* s = (const uint4*)p; RegWords r; r.q0 = s[0]; r.q1 = s[1]; r.q2 = s[2]; r.q3 = s[3]; r.q4 = s[4]; r.q5 = s[5]; r.q6 = s[6]; return r; }
__device__ __forceinline__ void reg_store(meme_alnreg* p, const RegWords& r) { uint4* d = (uint4*)p; d[0] = r.q0; d[1] = r.q1; d[2] = r.q2; d[3] = r.q3; d[4] = r.q4; d[5] = r.q5; d[6] = r.q6; }

// read r's records: [*base, *base + *n); a pair of offsets that is no span inside the record array gives no records (false)
__device__ __forceinline__ bool reg_span(const i64* reg_off, i64 r, i64 total_regs, i64* base, int* n) {
    const i64 s = reg_off[r], e = reg_off[r + 1];
    const bool ok = s >= 0 && e >= s && e <= total_regs && e - s <= INT_MAX;
    *base = ok ? s : 0;
    *n = ok ? (int)(e - s) : 0;
    return ok;
}

// a host form's records (nreads > 0, reg_off not null): reg_off starts at 0, does not decrease, no read has more than INT_MAX records, and the records are there
inline int reg_check_host(const char* who, const meme_alnreg* regs, const int64_t* reg_off, i64 nreads) {
    if (reg_off[0] != 0) { meme_set_error("%s: reg_off must start at 0", who); return MEME_E_ARG; }
    for (i64 r = 0; r < nreads; ++r)
        if (reg_off[r + 1] < reg_off[r] || reg_off[r + 1] - reg_off[r] > INT_MAX) { meme_set_error("%s: reg_off decreases (or spans more than 2^31 records) at read %lld", who, (long long)r); return MEME_E_ARG; }
    if (reg_off[nreads] > 0 && !regs) { meme_set_error("%s: null argument", who); return MEME_E_ARG; }
    return MEME_OK;
}
// a device form's arrays: none missing (rest: the stage's ctx, options and other outputs are there), the output records not the input records, both 16-byte aligned
inline int reg_check_device(const char* who, bool rest, const meme_alnreg* d_regs, const meme_alnreg* d_regs_out, const int64_t* d_reg_off, i64 nreads, i64 total_regs) {
    if (!rest || nreads < 0 || total_regs < 0 || (nreads > 0 && !d_reg_off) || (total_regs > 0 && (!d_regs || !d_regs_out || d_regs == d_regs_out))) {
        meme_set_error("%s: null argument (or the output records are the input records)", who);
        return MEME_E_ARG;
    }
    if (((uintptr_t)d_regs | (uintptr_t)d_regs_out) & 15) { meme_set_error("%s: the record arrays must be 16-byte aligned", who); return MEME_E_ARG; }
    return MEME_OK;
}

// ---- the steps of a host form: check, prepare, upload, reserve, launch, download, fill the result.  Every reserve of a call stands before its first launch, so
// a capacity refusal comes before any work; every copy goes from or to memory that outlives the call (the caller's arrays, pinned buffers of the ctx) ----
// upload: the records on their way into the stage's d_regs / d_reg_off; *total = the records.  reg_upload_host checks them first (reg_check_host); a stage with checks of
// its own between the two (pair scoring's n_pri) calls both: nothing is copied from the caller's arrays before the last check that can refuse them
inline int reg_upload(meme_ctx* ctx, const meme_alnreg* regs, const int64_t* reg_off, i64 nreads, DevBuf& d_regs, DevBuf& d_reg_off, i64* total) {
    *total = reg_off[nreads];
    const size_t rbytes = (size_t)*total * sizeof(meme_alnreg), obytes = (size_t)(nreads + 1) * 8;
    int rc;
    if ((rc = meme_buf_reserve(ctx, d_regs, rbytes + 64)) || (rc = meme_buf_reserve(ctx, d_reg_off, obytes))) return rc;
    if (*total) HIP_TRY(hipMemcpyAsync(d_regs.p, regs, rbytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_reg_off.p, reg_off, obytes, hipMemcpyHostToDevice, ctx->stream));
    return MEME_OK;
}
inline int reg_upload_host(meme_ctx* ctx, const char* who, const meme_alnreg* regs, const int64_t* reg_off, i64 nreads, DevBuf& d_regs, DevBuf& d_reg_off, i64* total) {
    const int rc = reg_check_host(who, regs, reg_off, nreads);
    return rc ? rc : reg_upload(ctx, regs, reg_off, nreads, d_regs, d_reg_off, total);
}
// the stage's device buffers of a call: each at least `bytes` and 64 more
struct DevNeed { DevBuf& buf; size_t bytes; };
inline int reg_reserve(meme_ctx* ctx, std::initializer_list<DevNeed> needs) {
    for (const DevNeed& n : needs) if (int rc = meme_buf_reserve(ctx, n.buf, n.bytes + 64)) return rc;
    return MEME_OK;
}
// download: `bytes` of `from` into the pinned `to`, in two steps around the launch -- the host buffers reserved (64 bytes more each), then the copies issued (none of 0 bytes)
struct Download { HostBuf& to; const DevBuf& from; size_t bytes; };
inline int reg_download_reserve(meme_ctx* ctx, std::initializer_list<Download> list) {
    for (const Download& d : list) if (int rc = meme_hostbuf_reserve(ctx, d.to, d.bytes + 64)) return rc;
    return MEME_OK;
}
inline int reg_download(meme_ctx* ctx, std::initializer_list<Download> list) {
    for (const Download& d : list) if (d.bytes) HIP_TRY(hipMemcpyAsync(d.to.p, d.from.p, d.bytes, hipMemcpyDeviceToHost, ctx->stream));
    return MEME_OK;
}
// timing: ctx->stream synchronised (what was downloaded is there), then the GPU time between the stage's two events
inline int reg_sync_ms(meme_ctx* ctx, Events<2>& ev, float* ms) {
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipEventElapsedTime(ms, ev[0], ev[1]));
    return MEME_OK;
}

// ---- tuning keys of the stages ----
// *_lds_recs, *_lds_keys: 0 and anything above the maximum mean the maximum
inline int tune_at_most(i64 v, int most) { return (int)(v > 0 && v < most ? v : most); }
// *_split: clamped to [0, g], the lanes of the light tier's group
inline int tune_split(i64 v, int g) { return (int)(v < 0 ? 0 : v > g ? g : v); }
// *_blocks: > 0 caps the grids, else 256 x 64 (grid_blocks' own cap)
inline i64 tune_grid_cap(i64 blocks) { return blocks > 0 ? blocks : 256 * 64; }
