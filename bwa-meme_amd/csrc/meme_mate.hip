// Mate rescue whole on the device (round 6): the POSING step of worker_sam's paired-end branch -- mem_sam_pe_batch_pre
// (reference src/bwamem_pair.cpp:660-716) with mem_matesw_batch_pre (:1060-1223) -- in front of the Smith-Waterman kernel that was here since
// round 3 (meme_kswv.hip: what mem_sam_pe_batch computes with kswv::getScores8 / getScores16).  Until now the binding ran the reference's own
// posing function for every worker batch on the host, copied the jobs' windows out of the 2-bit reference base by base and shipped ~600 bytes
// of sequence per job; the reads and the text are in HBM already.
//
// What the step does, per read pair and end i: the end's alignment records within pen_unpaired of its best one, at most max_matesw of them
// (:688-696); for each, the four orientations a mate could have (mem_infer_dir :58-65) minus those the insert-size statistics rule out
// (pes[r].failed) and those a record of the mate already explains (:1085-1091); for what is left the window of the reference the statistics
// point at, clamped to the strand and the reference sequence of its midpoint (bns_fetch_seq, src/bntseq.cpp:541-570); a job if the window
// lies on the record's sequence and holds min_seed_len bases (:1131).  The step's outputs are the jobs (in its own order: they are indexed by
// position) and `gar`, four job indices -- relative to the worker batch's first job -- or -1 per (end, record) looked at, which
// mem_sam_pe_batch_post reads to find its results (:1286-1296; -1 = compute it yourself).
//
// Mapping: one LANE per read (its records are few: two or three on average, 50 at most are looked at), two passes with a scan in between
// -- count (quads of gar, jobs, window bases, query bases per read), then write; a wavefront per job then unpacks the window from the 2-bit
// text and copies (or reverse-complements) the mate's bases, straight into the buffers k_kswv reads.  The jobs cross to the host once (32
// bytes each) for the sort into LDS classes the Smith-Waterman launches need; their sequences never do.
#include <string.h>
#include <vector>

#include "meme_common.h"
#include "meme_ext_rules.h"      // bns_clamp_to_mid
#include "meme_kswv_rules.h"     // every decision of the step

namespace {

struct MateAux { i64 rb; int read, is_rev; };                  // per job: window start (fwd+rc coordinate), the mate's read, reverse-complemented?

struct MateArgs {
    const meme_mate_reg* regs; const i64* reg_off; i64 n;       // n reads, the reads [first, first + n) of the resident batch (first even): pair p = reads 2p, 2p + 1
    i64 first;
    const i64* read_off;                                        // of the batch resident on the ctx
    meme_pestat pes[4];
    i64 l_pac; const i64* contig_off; const int* contig_len; int n_contigs;
    int a, pen_unpaired, max_matesw, min_seed_len, batch_reads;
    i64 *cntQ, *cntJ, *cntR, *cntY;                             // per read: (end, record) combinations looked at, jobs, window bases, query bases
    const i64 *offQ, *offJ, *offR, *offY;                       // their exclusive scans
    int32_t* gar; meme_kswv_job* jobs; MateAux* aux;
};

template <bool WRITE>
__global__ void __launch_bounds__(256) k_mate_plan(MateArgs A) {
    for (i64 r = (i64)blockIdx.x * 256 + threadIdx.x; r < A.n; r += (i64)gridDim.x * 256) {
        const i64 m = r ^ 1;                                    // the mate (the pair's other read)
        const meme_mate_reg* a = A.regs + A.reg_off[r];
        const int na = (int)(A.reg_off[r + 1] - A.reg_off[r]);
        const meme_mate_reg* ma = A.regs + A.reg_off[m];
        const int nm = (int)(A.reg_off[m + 1] - A.reg_off[m]);
        const int l_ms = (int)(A.read_off[A.first + m + 1] - A.read_off[A.first + m]);
        const int xtra = mate_xtra(l_ms, A.a, A.min_seed_len);
        i64 nq = 0, nj = 0, nr = 0;
        i64 q0 = 0, j0 = 0, r0 = 0, y0 = 0, jb = 0;
        if (WRITE) { q0 = A.offQ[r]; j0 = A.offJ[r]; r0 = A.offR[r]; y0 = A.offY[r]; jb = A.offJ[r / A.batch_reads * A.batch_reads]; }
        const int top = na ? a[0].score : 0;
        for (int j = 0; j < na && nq < A.max_matesw; ++j) {
            const meme_mate_reg rec = a[j];
            if (!(rec.score >= top - A.pen_unpaired)) continue;                          // :690
            const int skip = mate_skip_mask(A.pes, A.l_pac, rec.rb, ma, nm);
            int rid = -1;                                                                 // (carried from one orientation to the next, as in the reference)
            for (int o = 0; o < 4; ++o) {
                int idx = -1;
                if (mate_tries(skip, o)) {
                    const MateWindow W = mate_window(o, A.pes[o], rec.rb, l_ms, A.l_pac);
                    i64 rb = W.rb, re = W.re;
                    // bns_fetch_seq: the sequence of the window's midpoint, its strand
                    if (rb < re) rid = bns_clamp_to_mid(A.l_pac, A.contig_off, A.contig_len, A.n_contigs, (rb + re) >> 1, rb, re);
                    if (mate_is_job(rec.rid, rid, rb, re, A.min_seed_len)) {
                        if (WRITE) {
                            meme_kswv_job J;
                            J.idr = r0 + nr; J.idq = y0 + nj * l_ms; J.len1 = (int)(re - rb); J.len2 = l_ms; J.xtra = xtra; J.pad = 0;
                            A.jobs[j0 + nj] = J;
                            MateAux X; X.rb = rb; X.read = (int)(A.first + m); X.is_rev = W.is_rev;
                            A.aux[j0 + nj] = X;
                            idx = (int)(j0 + nj - jb);                                   // relative to the worker batch's first job: what the third step indexes with
                        }
                        ++nj; nr += re - rb;
                    }
                }
                if (WRITE) A.gar[4 * (q0 + nq) + o] = idx;
            }
            ++nq;
        }
        if (!WRITE) { A.cntQ[r] = nq; A.cntJ[r] = nj; A.cntR[r] = nr; A.cntY[r] = nj * l_ms; }
    }
}

// the sequences of the posed jobs, a wavefront per job: the window unpacked from the 2-bit fwd+rc text (what bns_get_seq returns, src/bntseq.cpp:515-539),
// the mate's bases as they are or reversed and complemented (:1111-1116)
__global__ void __launch_bounds__(256) k_mate_seq(const meme_kswv_job* __restrict__ jobs, const MateAux* __restrict__ aux, i64 n, const u64* __restrict__ pac,
                                                  const uint8_t* __restrict__ reads, const i64* __restrict__ read_off, uint8_t* __restrict__ ref, uint8_t* __restrict__ qer) {
    const i64 k = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= n) return;
    const int lane = threadIdx.x & 63;
    const meme_kswv_job J = jobs[k];
    const MateAux X = aux[k];
    uint8_t* r = ref + J.idr;
    for (int l = lane; l < J.len1; l += 64) {
        const i64 p = X.rb + l;
        r[l] = (uint8_t)text_base(pac, p);
    }
    const uint8_t* ms = reads + read_off[X.read];
    uint8_t* q = qer + J.idq;
    for (int l = lane; l < J.len2; l += 64) q[l] = mate_query_base(ms, J.len2, l, X.is_rev != 0);
}

// first gar entry and first job of every worker batch (batch b = reads [b * batch_reads, ...)), + the totals behind the last one
__global__ void k_mate_batch_offs(const i64* __restrict__ offQ, const i64* __restrict__ offJ, i64 n, int batch_reads, i64 nb, i64* __restrict__ gar_off, i64* __restrict__ job_off) {
    const i64 b = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (b > nb) return;
    const i64 r = b * batch_reads < n ? b * batch_reads : n;
    gar_off[b] = 4 * offQ[r];
    job_off[b] = offJ[r];
}

}  // namespace

extern "C" int meme_matesw_batch_host(meme_ctx* ctx, meme_ctx* reads_of, const meme_mate_reg* regs, const int64_t* reg_off, int64_t first_read, int64_t nreads, const meme_pestat* pes,
                                      const meme_contig* contigs, int32_t n_contigs, int64_t l_pac, const meme_mate_opt* opt, meme_mate_host_result* out) {
    static const char* const who = "meme_matesw_batch_host";
    if (!ctx || !reg_off || !pes || !contigs || n_contigs < 1 || !opt || !out || nreads < 0) { meme_set_error("%s: null argument", who); return MEME_E_ARG; }
    HIP_TRY(hipSetDevice(ctx->device));
    memset(out, 0, sizeof(*out));
    ctx->mate.last_nb = -1;                                     // (meme_matesw_last_device: nothing to hand out until this call has returned MEME_OK)
    if (nreads == 0) return MEME_OK;
    // the batch whose reads are named: this ctx's, or -- reads_of -- that of another ctx of the same GPU (a binding that runs this stage beside another one
    // on the ctx that seeded the batch: the bases are only read, device pointers are valid across the ctxs of a device)
    meme_ctx* const rc_ = reads_of ? reads_of : ctx;
    if (rc_->device != ctx->device) { meme_set_error("%s: the ctx that holds the reads is on another device", who); return MEME_E_ARG; }
    if (first_read < 0 || first_read + nreads > rc_->batch.last_seed_reads || !rc_->batch.reads_resident || !rc_->batch.reads.p || !rc_->batch.read_off.p) {
        meme_set_error("%s: reads [%lld, %lld) must lie in the batch resident on the ctx (a seeding call stages it; it holds %lld)", who, (long long)first_read, (long long)(first_read + nreads),
                       (long long)rc_->batch.last_seed_reads);
        return MEME_E_STATE;
    }
    if ((nreads & 1) || (first_read & 1)) { meme_set_error("%s: an odd number of reads (or an odd first read) is not a set of pairs", who); return MEME_E_ARG; }
    if (l_pac * 2 != ctx->idx.n) { meme_set_error("%s: l_pac does not match the loaded index", who); return MEME_E_ARG; }
    if (opt->batch_reads < 2 || (opt->batch_reads & 1) || opt->max_matesw < 0 || opt->a < 1 || opt->min_seed_len < 1) { meme_set_error("%s: bad options", who); return MEME_E_ARG; }
    const i64 nrec = reg_off[nreads];
    if (reg_off[0] != 0 || nrec < 0 || (nrec > 0 && !regs)) { meme_set_error("%s: bad record offsets", who); return MEME_E_ARG; }
    const i64 n = nreads, nb = (n + opt->batch_reads - 1) / opt->batch_reads;
    int rc;
    MateWs& M = ctx->mate;
    ContigTab ct(nullptr, 0);
    if ((rc = meme_contigs(ctx, "meme_matesw_batch_host: ", contigs, n_contigs, l_pac, &ct))) return rc;
    if ((rc = meme_hostbuf_reserve(ctx, ctx->h_ctr, 4 * 8)) || (rc = meme_buf_reserve(ctx, M.regs, (size_t)(nrec + 1) * sizeof(meme_mate_reg))) || (rc = meme_buf_reserve(ctx, M.reg_off, (size_t)(n + 1) * 8)) ||
        (rc = meme_buf_reserve(ctx, M.counts, MateCounts(nullptr, n).bytes)) || (rc = meme_buf_reserve(ctx, M.batch_off, (size_t)(nb + 1) * 16))) return rc;
    Events<2>& ev = ctx->kswv.ev;
    HIP_TRY(ev.ensure());
    if (nrec) HIP_TRY(hipMemcpyAsync(M.regs.p, regs, (size_t)nrec * sizeof(meme_mate_reg), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(M.reg_off.p, reg_off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    MateArgs A;
    memset(&A, 0, sizeof(A));
    A.regs = (const meme_mate_reg*)M.regs.p; A.reg_off = (const i64*)M.reg_off.p; A.n = n; A.first = first_read; A.read_off = (const i64*)rc_->batch.read_off.p;
    for (int o = 0; o < 4; ++o) A.pes[o] = pes[o];
    A.l_pac = l_pac; A.contig_off = ct.off; A.contig_len = ct.len; A.n_contigs = n_contigs;
    A.a = opt->a; A.pen_unpaired = opt->pen_unpaired; A.max_matesw = opt->max_matesw; A.min_seed_len = opt->min_seed_len; A.batch_reads = opt->batch_reads;
    const MateCounts mc(M.counts.p, n);
    A.cntQ = mc.cntQ; A.cntJ = mc.cntJ; A.cntR = mc.cntR; A.cntY = mc.cntY; A.offQ = mc.offQ; A.offJ = mc.offJ; A.offR = mc.offR; A.offY = mc.offY;
    HIP_TRY(hipEventRecord(ev[0], ctx->stream));
    hipLaunchKernelGGL((k_mate_plan<false>), dim3(grid_blocks(n, 256, 256 * 32)), dim3(256), 0, ctx->stream, A);
    for (int k = 0; k < 4; ++k) if ((rc = meme_scan_exclusive(ctx, mc.cntQ + k * (n + 1), mc.offQ + k * (n + 1), n))) return rc;
    const i64* tot = (const i64*)ctx->h_ctr.p;                                        // the four scans' totals
    for (int k = 0; k < 4; ++k) HIP_TRY(hipMemcpyAsync(ctx->h_ctr.as<i64>() + k, mc.offQ + k * (n + 1) + n, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const i64 nq = tot[0], nj = tot[1], ref_bytes = tot[2], qer_bytes = tot[3];
    if (nj > 0x7fffffff / 2 || 4 * nq > 0x7fffffff) { meme_set_error("%s: too many jobs in one call", who); return MEME_E_CAPACITY; }
    KswvWs& K = ctx->kswv;        // (k_kswv's jobs and sequences: written here, read there)
    if ((rc = meme_buf_reserve(ctx, M.gar, (size_t)(4 * nq + 4) * 4)) || (rc = meme_buf_reserve(ctx, M.aux, (size_t)(nj + 1) * sizeof(MateAux))) ||
        (rc = meme_buf_reserve(ctx, K.jobs, (size_t)(nj + 1) * sizeof(meme_kswv_job))) || (rc = meme_buf_reserve(ctx, K.ref, (size_t)ref_bytes + 64)) ||
        (rc = meme_buf_reserve(ctx, K.qer, (size_t)qer_bytes + 64)) || (rc = meme_hostbuf_reserve(ctx, M.h_gar, (size_t)(4 * nq + 4) * 4)) ||
        (rc = meme_hostbuf_reserve(ctx, M.h_batch_off, (size_t)(nb + 1) * 16)) || (rc = meme_hostbuf_reserve(ctx, M.h_jobs, (size_t)(nj + 1) * sizeof(meme_kswv_job)))) return rc;
    A.gar = (int32_t*)M.gar.p; A.jobs = (meme_kswv_job*)K.jobs.p; A.aux = (MateAux*)M.aux.p;
    hipLaunchKernelGGL((k_mate_plan<true>), dim3(grid_blocks(n, 256, 256 * 32)), dim3(256), 0, ctx->stream, A);
    if (nj) hipLaunchKernelGGL(k_mate_seq, dim3((unsigned)((nj + 3) / 4)), dim3(256), 0, ctx->stream, (const meme_kswv_job*)K.jobs.p, (const MateAux*)M.aux.p, nj, ctx->idx.pac,
                               (const uint8_t*)rc_->batch.reads.p, (const i64*)rc_->batch.read_off.p, (uint8_t*)K.ref.p, (uint8_t*)K.qer.p);
    i64* d_goff = (i64*)M.batch_off.p;
    i64* d_joff = d_goff + (nb + 1);
    hipLaunchKernelGGL(k_mate_batch_offs, dim3((unsigned)((nb + 256) / 256)), dim3(256), 0, ctx->stream, A.offQ, A.offJ, n, opt->batch_reads, nb, d_goff, d_joff);
    HIP_TRY(hipGetLastError());
    if (nq) HIP_TRY(hipMemcpyAsync(M.h_gar.p, M.gar.p, (size_t)(4 * nq) * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(M.h_batch_off.p, M.batch_off.p, (size_t)(nb + 1) * 16, hipMemcpyDeviceToHost, ctx->stream));
    if (nj) HIP_TRY(hipMemcpyAsync(M.h_jobs.p, K.jobs.p, (size_t)nj * sizeof(meme_kswv_job), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipEventRecord(ev[1], ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    float pose_ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&pose_ms, ev[0], ev[1]));
    meme_kswv_host_result R;
    memset(&R, 0, sizeof(R));
    if (nj) {
        meme_bsw_opt bo;
        memset(&bo, 0, sizeof(bo));
        bo.a = opt->a; bo.b = opt->b; bo.o_del = opt->o_del; bo.e_del = opt->e_del; bo.o_ins = opt->o_ins; bo.e_ins = opt->e_ins;
        if ((rc = meme_kswv_run(ctx, (const meme_kswv_job*)M.h_jobs.p, nj, nullptr, ref_bytes, nullptr, qer_bytes, &bo, true, &R))) return rc;
    }
    out->nreads = n; out->nbatches = nb; out->njobs = nj; out->n_gar = 4 * nq;
    out->gar = (const int32_t*)M.h_gar.p; out->gar_off = (const int64_t*)M.h_batch_off.p; out->job_off = (const int64_t*)M.h_batch_off.p + (nb + 1);
    out->jobs = (const meme_kswv_job*)M.h_jobs.p; out->res = R.res; out->pose_ms = pose_ms; out->kernel_ms = R.kernel_ms;
    M.last_nb = nb; M.last_njobs = nj;
    return MEME_OK;
}

extern "C" int meme_matesw_last_device(meme_ctx* ctx, meme_rescue_jobs_in* view) {
    if (!ctx || !view) { meme_set_error("meme_matesw_last_device: null argument"); return MEME_E_ARG; }
    const MateWs& M = ctx->mate;
    if (M.last_nb < 0) { meme_set_error("meme_matesw_last_device: no meme_matesw_batch_host call on this ctx whose results are still on the device"); return MEME_E_STATE; }
    view->gar = (const int32_t*)M.gar.p; view->gar_off = (const int64_t*)M.batch_off.p; view->job_off = (const int64_t*)M.batch_off.p + (M.last_nb + 1);
    view->nbatches = M.last_nb; view->res = (const meme_kswr*)ctx->kswv.res.p; view->njobs = M.last_njobs;
    return MEME_OK;
}
