// Shared declarations of the HIP backend (gfx950 / MI355X only -- no portability layer).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "meme_hip.h"

typedef uint64_t u64;
typedef int64_t i64;

// ---- HBM layout of the index ---------------------------------------------------------------------
// One suffix-array slot: the first 32 bases of the suffix as an integer whose unsigned order is the
// lexicographic order (first base in bits 63..62, T-filled past the text end), plus the text position.
// 16-byte aligned: one probe = one dwordx4 load = one 64-B HBM sector.
struct __attribute__((aligned(16))) SaEnt {
    u64 key;
    u64 pos;
};

struct RmiRec {   // on-disk P-RMI record (reference src/LearnedIndex_seeding.cpp:197-206)
    double icpt;
    double slope;
    u64 err;
};

struct Rmi32 {    // the same record padded to 32 bytes in HBM: a lookup never straddles a 128-byte line
    double icpt;
    double slope;
    u64 err;
    u64 pad;
};

struct DevIndex {
    i64 n = 0;                 // sa_num = 2 * l_pac
    const SaEnt* sa = nullptr;
    const u64* pac = nullptr;  // 2-bit text, base i in bits (62 - 2*(i&31)) of word i>>5
    const Rmi32* l2 = nullptr;
    const Rmi32* l1 = nullptr;
    i64 n_l2 = 0, n_l1 = 0;
    int shift = 64;            // key >> shift = leaf index
    // plcp[u] = min(255, longest common prefix of the suffix at TEXT position u with either of its suffix-array neighbours): the depth
    // down to which that suffix is not alone in its suffix-array interval.  Derived from sa + pac when an index is staged
    // (k_build_plcp); what the re-seeding verifier (k_reseed) walks instead of searching.  1 byte per suffix.
    const uint8_t* plcp = nullptr;
};

// Workspaces free themselves (a ctx is destroyed with its device current and its streams idle) and cannot be copied.
template <bool HOST> struct Buf {   // growable device workspace (meme_buf_reserve) / pinned host staging (meme_hostbuf_reserve)
    void* p = nullptr;
    size_t cap = 0;
    Buf() = default;
    Buf(const Buf&) = delete; Buf& operator=(const Buf&) = delete;
    ~Buf() { if (p) (void)(HOST ? hipHostFree(p) : hipFree(p)); }
    template <class T> T* as() const { return (T*)p; }
};
typedef Buf<false> DevBuf;
typedef Buf<true> HostBuf;
static_assert(!std::is_copy_constructible<DevBuf>::value && !std::is_copy_assignable<DevBuf>::value && !std::is_copy_constructible<HostBuf>::value &&
              !std::is_copy_assignable<HostBuf>::value, "a workspace owns its memory: a copy would free it twice");
template <int N> struct Events {    // events of a stage, created on first use, destroyed with the stage
    hipEvent_t e[N] = {};
    Events() = default;
    Events(const Events&) = delete; Events& operator=(const Events&) = delete;
    ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    hipEvent_t& operator[](int i) { return e[i]; }
    hipError_t ensure() { for (hipEvent_t& x : e) if (!x) { const hipError_t r = hipEventCreate(&x); if (r != hipSuccess) return r; } return hipSuccess; }   // whichever are missing
};
struct Stream {                     // a stream besides the caller's, created on first use, destroyed with its owner
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream&) = delete; Stream& operator=(const Stream&) = delete;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
};

// Packed layouts: typed arrays carved out of one allocation in order.  The same code gives the total bytes (base == nullptr) and the pointers.
struct Carve {
    unsigned char* base;
    size_t bytes = 0;
    explicit Carve(void* b) : base((unsigned char*)b) {}
    template <class T> T* take(size_t count, size_t align = 1) { bytes = (bytes + align - 1) / align * align; T* q = base ? (T*)(base + bytes) : nullptr; bytes += count * sizeof(T); return q; }
    i64* col(i64 n) { return take<i64>((size_t)n + 1); }   // one column of n + 1 values
};
struct ContigTab {     // ContigCache::dev: offset[n], len[n], is_alt[n] (chaining and record finishing read it), 64 bytes of padding
    i64* off; int* len; unsigned char* alt; size_t bytes;
    ContigTab(void* base, i64 n) { Carve c(base); off = c.take<i64>(n); len = c.take<int>(n); alt = c.take<unsigned char>(n + 64); bytes = c.bytes; }
};
struct ChainCounts {   // per read, then the reads each wavefront launch takes (5 counters)
    i64 *chain_off, *seed_off, *nch, *nsd; int* tree; unsigned char* fb; unsigned long long* route; size_t bytes;
    ChainCounts(void* base, i64 n) { Carve c(base); chain_off = c.col(n); seed_off = c.col(n); nch = c.col(n); nsd = c.col(n); tree = c.take<int>(n); fb = c.take<unsigned char>(n + 64);
                                     route = c.take<unsigned long long>(8, 16); bytes = c.bytes; }
};
struct ChainLists {    // list, work and work offsets of the five wavefront launches, read classes
    i64 *list[5], *work[5], *woff[5]; unsigned char* cls; size_t bytes;
    ChainLists(void* base, i64 n) { Carve c(base); for (int k = 0; k < 5; ++k) { list[k] = c.col(n); work[k] = c.col(n); woff[k] = c.col(n); } cls = c.take<unsigned char>(n + 64); bytes = c.bytes; }
};
enum { EXT_L = 0, EXT_R = 1, EXT_B = 2 };   // ExtCounts columns: left jobs, right jobs, sequence bytes
struct ExtCounts {     // per read cnt[k], their scans off[k], seeds selected per round and its scan.  The multi-slab path copies the three off columns as one block: adjacent(), checked there
    i64 *cnt[3], *off[3], *cntS, *offS; size_t bytes;
    ExtCounts(void* base, i64 n) { Carve c(base); for (i64*& q : cnt) q = c.col(n); for (i64*& q : off) q = c.col(n); cntS = c.col(n); offS = c.col(n); bytes = c.bytes; }
    bool adjacent(i64 n) const { return off[1] == off[0] + (n + 1) && off[2] == off[1] + (n + 1); }
};
struct CountScan {     // ExtWs::flt_cnt (seeds the filter keeps per read; the scan is the new seed_off) and ExtWs::live_cnt (surviving records per read): counts, their scan
    i64 *cnt, *off; size_t bytes;
    CountScan(void* base, i64 n) { Carve c(base); cnt = c.col(n); off = c.col(n); bytes = c.bytes; }
};
struct ExtRetry {      // ExtWs::retry: the jobs a fold sends to the next band width, attempts alternating between the halves (nmax: the larger side's jobs)
    meme_seqpair* half[2]; size_t bytes;
    ExtRetry(void* base, i64 nmax) { Carve c(base); for (meme_seqpair*& q : half) q = c.take<meme_seqpair>((size_t)nmax + 1); bytes = c.bytes; }
};
struct ExtRounds {     // extension in rounds: per-read state, reads still active, seeds selected
    int4* state; uint8_t* act; uint8_t* sel; size_t bytes;
    ExtRounds(void* base, i64 n, i64 seeds) { Carve c(base); state = c.take<int4>(n + 1); act = c.take<uint8_t>(n + 1); sel = c.take<uint8_t>(seeds + 64); bytes = c.bytes; }
};
struct GcigCols {      // per CIGAR job: sizes, scans, the DP list and its classes; then the first bad job
    i64 *zsz, *csz, *zoff, *coff, *ncig, *ooff, *msz, *moff, *psz, *poff, *isdp, *dpoff, *dplist, *is16, *o16, *is32, *o32, *is64, *o64, *bad; size_t bytes;
    GcigCols(void* base, i64 n) { Carve c(base); zsz = c.col(n); csz = c.col(n); zoff = c.col(n); coff = c.col(n); ncig = c.col(n); ooff = c.col(n); msz = c.col(n); moff = c.col(n);
        psz = c.col(n); poff = c.col(n); isdp = c.col(n); dpoff = c.col(n); dplist = c.col(n); is16 = c.col(n); o16 = c.col(n); is32 = c.col(n); o32 = c.col(n); is64 = c.col(n);
        o64 = c.col(n); bad = c.take<i64>(8); bytes = c.bytes; }
};
struct BswSort {       // query-length sort of a banded-SW batch (ints, cleared as one block): histogram, exclusive offsets (+ total), scatter cursors, the longest query of the
                       // pairs the lane kernel cannot take, the kernels' tickets
    int *hist, *offs, *cursor, *maxq; unsigned int* tickets; size_t bytes;
    BswSort(void* base, int keys) { Carve c(base); hist = c.take<int>(keys); offs = c.take<int>(keys + 1); cursor = c.take<int>(keys); maxq = c.take<int>(1); tickets = c.take<unsigned int>(30); bytes = c.bytes; }
};
struct MateCounts {    // gar entries, jobs, window bases and query bases per read, and their scans
    i64 *cntQ, *cntJ, *cntR, *cntY, *offQ, *offJ, *offR, *offY; size_t bytes;
    MateCounts(void* base, i64 n) { Carve c(base); cntQ = c.col(n); cntJ = c.col(n); cntR = c.col(n); cntY = c.col(n); offQ = c.col(n); offJ = c.col(n); offR = c.col(n); offY = c.col(n); bytes = c.bytes; }
};
struct SamCols {       // per record slot: scratch bound, its scan, text length, its scan; then the first bad record
    i64 *bound, *soff, *len, *toff, *bad; size_t bytes;
    SamCols(void* base, i64 n) { Carve c(base); bound = c.col(n); soff = c.col(n); len = c.col(n); toff = c.col(n); bad = c.take<i64>(8); bytes = c.bytes; }
};
// ---- per-stage workspaces of a ctx -----------------------------------------------------------------
// What a seeding call leaves on the ctx for the stages behind it.  Invariant: only the calls that set a new batch (the seeding calls, and
// meme_chain_batch_host, which brings its seeds in place of one) reserve these buffers; chaining, extension, CIGAR, SAM and mate calls only
// read them.  meme_matesw_batch_host(..., reads_of, ...) relies on this when it reads another ctx's batch.
struct ResidentBatch {
    DevBuf reads, read_off, packed, smems, hits, smem_off, hit_off;
    i64 last_seed_reads = 0;           // reads of the batch whose seeds are in smems / hits (input of meme_chain_last_batch_host)
    i64 last_seed_max_len = 0;         // longest read of that batch
    i64 packed_reads = 0;              // reads in `packed` and their layout (PackGeom: W, MW, stride), for meme_debug_packed_reads
    int packed_geom[3] = {0, 0, 0};
    bool reads_resident = false;       // reads holds the bases of that batch (false after meme_chain_batch_host: seeds brought by the caller)
};
// a seeding counter set (u64): slot cursor of the tier, searches, reads left for the next tier (the length of its overflow list), window loads, eight diagnostic sums
// (SEED_PROF, or RESEED_PROF's census), searches of the re-seeding kernels' lanes, length of the pending list, the two blocked-region cursors; then what
// meme_debug_reseed_counts reports: the length of the blocked list each batch search met (one per round), the blocked regions' lane searches by the region's
// stage, how many of them ended without an interval / walked a run for one, and their probes of a neighbour slot outside the cached window; last, the read cursor
// of tier 0's round-3 launch and the third-round searches it ran twice (key-only compares could not decide them)
enum { SEED_CTR_SLOT = 0, SEED_CTR_SEARCHES = 1, SEED_CTR_OVERFLOW = 2, SEED_CTR_WINDOWS = 3, SEED_CTR_PROF = 4, SEED_CTR_LANE = 12, SEED_CTR_PEND = 13, SEED_CTR_BLK = 14, SEED_CTR_BLK_OUT = 15,
       SEED_CTR_RS_ROUND = 16, SEED_CTR_RS_STAGE = 24, SEED_CTR_RS_NOINTV = 27, SEED_CTR_RS_WALKED = 28, SEED_CTR_RS_NBPROBE = 29, SEED_CTR_SLOT3 = 30, SEED_CTR_R3_REPEAT = 31, SEED_CTRS = 32 };
constexpr int RESEED_MAX_ROUNDS = SEED_CTR_RS_STAGE - SEED_CTR_RS_ROUND;
enum { SEED_EV_PACK0, SEED_EV_PACK1, SEED_EV_SEARCH0, SEED_EV_SEARCH1, SEED_EV_RESEED0, SEED_EV_GATHER0, SEED_EV_GATHER1, SEED_EVS };   // SeedWs::ev: begin / end of packing, of a tier's search, begin of re-seeding, begin / end of offsets + gather
struct SeedWs {
    DevBuf slots[3], ovf[2];           // SMEM slots of a tier; reads that overflow it (tier & 1)
    DevBuf slot_cnt, slot_hits, slot_loc, counters, pend, blk;
    DevBuf carry;                      // per read, from tier 0's rounds-1/2 launch to its round-3 launch: searches | windows << 32, or "sent to the overflow list"
    long long r3_counts[MEME_R3_COUNTS] = {0};   // the last seeding call: did tier 0 run in two launches, third-round searches run twice (meme_debug_seed_r3_counts)
    bool r3_valid = false;
    long long reseed_counts[SEED_CTRS - SEED_CTR_RS_ROUND] = {0};   // the re-seeding counters of the last seeding call (meme_debug_reseed_counts); valid while reseed_rounds > 0
    int reseed_rounds = 0;
    HostBuf h_smems, h_hits, h_smem_off, h_hit_off;   // results of meme_seed_batch_host
    unsigned long long* counter_set(int cset) { return (unsigned long long*)counters.p + SEED_CTRS * cset; }   // two sets: an overflow tier may run beside the re-seeding kernels
    Events<SEED_EVS> ev;
    Stream emit; Events<2> emit_ev;    // k_reseed_emit runs beside the blocked regions' rounds: its stream, fork [0] and join [1]
};
struct ChainWs {
    DevBuf ch1, sd1, hdr, frac, counts, chains, seeds, lists;            // lane-tier chains / seeds, read headers, frac_rep, ChainCounts, packed chains / seeds, ChainLists
    DevBuf wave[5];                                                       // scratch sets of the five wavefront launches
    HostBuf h_chain_off, h_chains, h_seed_off, h_seeds, h_tree, h_frac, h_fallback;
    Events<5> ev;
    const i64* chain_off() const { return (const i64*)counts.p; }   // (ChainCounts)
    const i64* seed_off(i64 n) const { return ChainCounts(counts.p, n).seed_off; }
};
enum { EXT_CTR_RETRY = 0, EXT_CTR_FLT_JOBS = 2, EXT_CTR_CENSUS = 8, EXT_CTR_HEAVY = 24, EXT_CTR_BYTES = 256 };   // ExtWs::counters (u64); the census takes 11
struct ExtWs {
    DevBuf rmax, regs, order, counts, pairs_l, pairs_r, retry, seq, counters;   // counts: ExtCounts; retry: ExtRetry
    DevBuf flt_sc, flt_jobs, flt_cnt, flt_seeds, flt_score, flt_hsp;           // the seed filter's: scores, jobs, CountScan (the scan = new seed offsets), kept seeds, their scores, thresholds
    DevBuf live_cnt, live_regs, rounds, heavy;                                 // surviving records (CountScan, packed), ExtRounds, the heavy reads
    HostBuf h_reg_off, h_regs; Events<2> ev;
};
struct BswWs { DevBuf pairs, refb, qerb, order, ws, hist; Events<2> ev; };   // hist: BswSort; ev: begin / end of the last meme_bsw_launch
struct GcigWs {        // cols: GcigCols; cig: CIGAR scratch, ops: packed; nm: nm + mdlen
    DevBuf jobs, cols, z, cig, res, ops, md, nm, md_packed, cjobs, cres; HostBuf h_res, h_ops, h_md; Events<2> ev;
};
struct KswvWs {        // mate rescue poses into jobs, ref and qer; k_kswv reads them
    DevBuf jobs, order, ref, qer, res, rowmax, rm_off; HostBuf h_res; Events<2> ev;
};
struct MateWs {        // counts: MateCounts; batch_off: gar and job offsets of the worker batches
    DevBuf regs, reg_off, counts, gar, aux, batch_off; HostBuf h_gar, h_batch_off, h_jobs;
    i64 last_nb = -1, last_njobs = 0;  // the last meme_matesw_batch_host call that returned MEME_OK: its worker batches (-1: none, or a kswv call has taken KswvWs::res since) and jobs
};
struct SamWs {         // cols: SamCols; contigs: contig name offsets + names + read group
    DevBuf names, name_off, quals, recs, blob, cols, scratch, text, contigs; HostBuf h_text_off, h_text; Events<2> ev;
};

struct PrimaryWs {     // regs / reg_off / out / n_pri / mapq / status: the host form's staging; sorted: a heavy read's records in the first order; rank: its ranks in the second; list: the heavy
                       // reads, counter: how many; logtab: log((double)k), k < 65536, by the host's libm
    DevBuf regs, reg_off, out, n_pri, mapq, status, sorted, rank, list, counter, logtab; HostBuf h_regs, h_n_pri, h_mapq, h_status; Events<2> ev;
    bool log_ready = false;
};

struct PairWs {        // regs / reg_off / n_pri / res / status / counter: the host form's staging (res: score, sub, n_sub, n_cand and z, six ints a pair); keys: a heavy pair's sorted keys
                       // behind the LDS cap; list: the heavy pairs; tab: PairDirs and the penalty table, h_tab what it is copied from (tab_ev: the copy has passed)
    DevBuf regs, reg_off, n_pri, res, status, counter, keys, list, tab; HostBuf h_res, h_status, h_tab; Events<2> ev; Events<1> tab_ev;
    bool tab_in_flight = false;
};

struct DecideWs {      // regs / reg_off / n_pri / in / in_status / res / status / counter: the host form's staging (in: the pair stage's score, sub, n_sub and z, five ints a pair; res: path,
                       // q_pe, flag, sel, q_se and alt, nine ints a pair); list: the heavy pairs
    DevBuf regs, reg_off, n_pri, in, in_status, res, status, counter, list; HostBuf h_regs, h_res, h_status; Events<2> ev;
};

struct RescueWs {      // regs / reg_off / ums / rlen / gar / gar_off / job_off / res / out / reg_off_out / status / counters: the host form's staging; cnt_a / off_a: records of a read
                       // that are looked at, and the scan; cap / off_c: records a list can come to hold, and the scan (where its records stand in `stage` before the pack);
                       // cnt: records a list is left with; list: the wavefront tier's lists; cols_l / cols_c: the columns of lists too large for LDS, at off_c
    DevBuf regs, reg_off, ums, rlen, gar, gar_off, job_off, res, out, reg_off_out, status, counters, stage, cnt_a, off_a, cap, off_c, cnt, list, cols_l, cols_c;
    HostBuf h_regs, h_reg_off, h_status; Events<2> ev;
};

struct FinishWs {      // regs / reg_off / out / reg_off_out / ums / status / counters: the host form's staging; stage: the records a read keeps, at the read's input offsets, before the
                       // pack; cnt: records kept per read; live / first: live records of a read and the first of them; list: the wavefront tier's reads; cols_l / cols_c: the
                       // columns of reads too large for LDS
    DevBuf regs, reg_off, out, reg_off_out, ums, status, counters, stage, cnt, live, first, list, cols_l, cols_c;
    HostBuf h_regs, h_reg_off, h_ums, h_status; Events<2> ev;
};

// The contig table of a ctx (meme_contigs): one for every stage that takes contigs -- chaining and extension, mate rescue, record finishing, pair scoring.
// dev: ContigTab; host: the pinned image it was copied from; from / l_pac: the caller's array and genome length it was built from (l_pac -1: nothing valid).
// Invariant: dev is only ever overwritten by a copy on ctx->stream issued after that stream has been synchronised, and that copy has passed before meme_contigs
// returns; every kernel that reads dev runs on ctx->stream, or on a side stream that its call joins before it returns (SideGuard in meme_chain_run).  So a
// new table never meets a reader of the old one, and host is idle whenever it is rewritten.  A ctx is driven by one host thread at a time.
struct ContigCache {
    DevBuf dev; HostBuf host;
    std::vector<meme_contig> from; i64 l_pac = -1;
};

struct SideStreams {   // beside ctx->stream: the routed chaining tiers, the early overflow tier of seeding (meme_side_stream creates stream i with its event)
    Stream st[3];
    Events<3> done;    // done[i]: what was launched on st[i] has finished
    Events<1> fork;    // recorded on ctx->stream where the side streams start
};

struct meme_ctx {
    int device = 0;
    int n_cus = 256;                   // compute units of the device (cached: hipGetDeviceProperties is slow)
    DevIndex idx;
    bool owns_index = false;
    std::vector<std::pair<void*, size_t>> owned;   // device allocations of the index (pointer, bytes)
    void* plcp_aux = nullptr;                      // the plcp table of an attached index (meme_index_attach: the arrays are the caller's, this is ours)
    // workspaces (scan_tmp: tiles of the prefix sums, meme_scan_exclusive and the seeding gather)
    ResidentBatch batch;
    DevBuf scan_tmp;
    ContigCache contigs;
    HostBuf h_ctr;                     // where a call's counters land on the host, read behind the call's own synchronise (never a stack variable: an error return
                                       // between the copy and the synchronise would leave the copy writing into a dead frame)
    ChainWs chain; ExtWs ext; BswWs bsw; GcigWs gcig; KswvWs kswv; MateWs mate; SamWs sam; PrimaryWs primary; PairWs pair; DecideWs decide; FinishWs finish; RescueWs rescue; SeedWs seed;
    // Streams.  Order of destruction: meme_ctx_destroy synchronises every stream of the ctx; then the members go in reverse order of declaration, so the streams
    // and their fork / join events -- these two and, last member of the last workspace, the seeding stage's -- are destroyed BEFORE any DevBuf / HostBuf above is
    // freed.  A new stream holder goes below the buffers too: here, or last in SeedWs.  (A stage's timing events go with the stage; they are idle by then.)
    Stream stream;
    SideStreams side;
    // tuning
    i64 seed_blocks = 0;               // 0 = auto
    i64 helper_blocks = 0;             // cap on the grids of the read packer, the offsets scan and the hit gather (0 = none)
    i64 smem_cap = 128;                // per-read SMEM slots in the search kernel's scratch (tier 0; 3 KB per read.  With 64 a handful of
                                       // the benchmark's 10 M reads overflowed and their sequential re-run cost every step 1.9 ms)
    i64 group_lanes = 4;               // lanes per read in the search kernel (4, 8, 16, 32)
    i64 seed_blocks_per_cu = 5;
    i64 max_batch = 0;                 // > 0: the batch calls behind seeding (extension, global alignment) refuse more reads / jobs than this with
                                       // MEME_E_CAPACITY, as they do when their scratch would not fit: a caller's memory bound, and how the tests reach that path
    i64 ext_slab_jobs = 8 << 20;       // the extension stage poses and aligns its jobs in slabs of whole reads: at most this many jobs per side and ext_slab_bytes of job sequence each, and at
    i64 ext_slab_bytes = (i64)3 << 29; // least one read (SeqPair offsets are 32-bit).  ext_slab_jobs has a tuning key: a bound, and how the tests reach the multi-slab path
    i64 ext_split = 1;                 // 1: the extension stage's read-walking kernels run eight lanes per read for reads with at most 8 chained seeds, a wavefront per read for the rest; 0: a wavefront per read
    i64 bsw_circ = 1;                  // 1: lane-per-pair banded SW of queries longer than 2w + 2 columns keeps its columns in a ring (k_bsw_lane_circ); 0: a word per query column
    i64 sam_max_batch = 0;             // > 0: meme_sam_format_batch_host refuses more record slots than this with MEME_E_CAPACITY (the caller then formats in pieces)
    i64 primary_split = 8;             // primary marking: reads with more records than this go to the wavefront-per-read tier (0: every non-empty read; at most 8, the lanes of the light tier's group)
    i64 primary_blocks = 0;            // > 0: cap on the workgroups of the primary-marking kernels (0 = none)
    i64 pair_split = 8;                // pair scoring: pairs with more keys (records of both ends that take part) than this go to the wavefront-per-pair tier (0: every non-empty pair; at most 8)
    i64 pair_blocks = 0;               // > 0: cap on the workgroups of the pair-scoring kernels (0 = none)
    i64 pair_lds_keys = 0;             // > 0: the wavefront tier keeps this many sorted keys of a pair in LDS, the rest in HBM (0, and anything above it: 512)
    i64 decide_split = 64;             // pairing decision: pairs whose two ends hold more records than this go to the wavefront-per-pair tier (0: every pair with a record; at most 1 << 20;
                                       // 64: the fastest of 0, 8, 16, 32, 64 on the production-shaped batch, profiles/decide_stage.md)
    i64 decide_blocks = 0;             // > 0: cap on the workgroups of the pairing-decision kernels (0 = none)
    i64 finish_blocks = 0;             // > 0: cap on the workgroups of the record-finishing kernels (0 = none)
    i64 finish_lds_recs = 0;           // > 0: reads handed over with more records than this are walked in HBM by the wavefront tier (0, and anything above it: 128)
    i64 rescue_blocks = 0;             // > 0: cap on the workgroups of the mate-rescue record kernels (0 = none)
    i64 rescue_lds_recs = 0;           // > 0: lists that can come to hold more records than this are walked in HBM by the wavefront tier (0, and anything above it: 128)
    i64 ext_live_only = 0;             // 1: meme_extend_last_batch_host hands over the surviving records only (qe > qb: what src/bwamem.cpp:1680-1693 keeps)
    i64 ext_rounds = 1;                // with ext_live_only: rounds of one seed per read before everything still ahead is extended at once (0: the reference's batch, then compaction)
    i64 gcig_groups = 1;               // 1: CIGAR jobs with bands of at most 16 / 32 / 64 columns run 4 / 2 / 1 to a wavefront as one chunk per row (k_gcig_grp); 0: a wavefront each, 64-column chunks
    i64 gcig_zcap = -1;                // >= 0: bytes of LDS per CIGAR job for its backtrack matrix / window (default: 8192 where a typical matrix of the batch fits, else 2048)
    i64 ext_census = 0;                // 1: the extension stage counts its exact-prefix jobs (a measurement, profiles/r05_bsw.md)
    i64 seed_defer = 1;                // 1: re-seeding regions of unique SMEMs are verified on the plcp table (k_reseed) instead of searched
    i64 seed_r3_split = 1;             // tier 0 with three rounds: 1 = the third round in a k_seed launch of its own behind rounds 1-2, its searches on the keys alone first;
                                       // 0 = one launch for all three rounds
    i64 chain_light_hits = 32;         // reads with more hits to walk skip the lane-per-read tier: LDS tier at once, beside it
    i64 chain_lane_hits = 256;         // hits per read the lane-per-read chaining tier walks; reads with more go to the wavefront tiers at once
    i64 chain_wave_tiers = 1;          // 0: the chaining stage skips the LDS tier (everything beyond the lane tier through the B-tree tier; tests)
    i64 sa_chunk = (i64)1 << 28;       // meme_sa_build_device sorts the four-base buckets in groups of at most this many suffixes (a bucket alone may exceed it) ...
    i64 sa_piece = (i64)1 << 28;       // ... and looks for the padding entries in pieces of this many slots.  Both have tuning keys: bounds of the workspace, and how the tests reach the
                                       // multi-group and multi-piece paths with small texts; same array
    i64 bsw_blocks = 0;
    i64 bsw_lane_min_pairs = 32768;   // batches at least this big use the lane-per-pair kernel (throughput); smaller ones the
                                       // lanes-per-pair kernel (latency: a lone pair takes ~6 ms on one lane, ~0.3 ms on 64)
    // what the last suffix-array build on this ctx did (meme_debug_sa_stats); valid after a build that returned MEME_OK
    bool sa_stats_valid = false;
    long long sa_stats[MEME_SA_STATS] = {0};
    // timings
    i64 sam_text_reads = 0;            // reads of the batch whose names / qualities meme_sam_stage_text staged (0: none)
    bool sam_has_quals = false;
    meme_timings tm = {};
};

void meme_set_error(const char* fmt, ...);
int meme_buf_reserve(meme_ctx* ctx, DevBuf& b, size_t bytes);
// side stream i of the ctx with its "done" event, and the fork event, created on first use
int meme_side_stream(meme_ctx* ctx, int i);
int meme_hostbuf_reserve(meme_ctx* ctx, HostBuf& b, size_t bytes);
// workgroups of a grid-stride launch over `items`, `per` to a workgroup: at least one, at most `cap` (256 x 64: 64 per CU of a 256-CU device)
inline unsigned grid_blocks(i64 items, int per, i64 cap = 256 * 64) { i64 b = (items + per - 1) / per; return (unsigned)(b < cap ? (b < 1 ? 1 : b) : cap); }
// the ctx's contig table for these contigs (ContigCache).  The array and l_pac of the call before: the resident table, no copy, no synchronisation.  Anything else:
// ctx->stream synchronised, the contigs checked (ascending, inside the forward strand of an l_pac-base genome; the error message starts with `prefix`), staged,
// synchronised again, remembered.  After a refusal nothing is remembered: the next call checks again.
int meme_contigs(meme_ctx* ctx, const char* prefix, const meme_contig* contigs, int32_t n_contigs, i64 l_pac, ContigTab* out);
// the ctx's table of logarithms, log((double)k) for k < 65536 by the host's libm (PrimaryWs::logtab): staged on first use, which synchronises ctx->stream once (meme_primary.hip)
int meme_logtab(meme_ctx* ctx, const double** d_tab);
// exclusive prefix sum of n 64-bit counts into out[0..n] (out[n] = total), asynchronous on ctx->stream (meme_scan.hip)
int meme_scan_exclusive(meme_ctx* ctx, const i64* d_in, i64* d_out, i64 n);
// the same, and the total on its way to *h_total (an asynchronous 8-byte copy: the caller synchronises ctx->stream before reading it)
int meme_scan_total(meme_ctx* ctx, const i64* d_in, i64* d_out, i64 n, i64* h_total);
// false: growing a workspace that holds `have` bytes to `need` would take more than half of the free HBM (*free_b, for the message); the caller refuses with MEME_E_CAPACITY
inline bool meme_fits_free_hbm(size_t need, size_t have, size_t* free_b) { size_t total_b = 0; return need <= have || hipMemGetInfo(free_b, &total_b) != hipSuccess || need <= *free_b / 2 + have; }
// the banded-SW kernels on device-resident pairs, no host synchronisation (meme_bsw.hip); host_maxq = an upper bound of the query lengths or -1
int meme_bsw_launch(meme_ctx* ctx, meme_seqpair* d_pairs, const uint8_t* d_ref, const uint8_t* d_qer, int npairs, int w, const meme_bsw_opt* opt,
                    int host_maxq);
// GPU time of the last meme_bsw_launch on the ctx, once ctx->stream has passed it
hipError_t meme_bsw_last_ms(meme_ctx* ctx, float* ms);
// local alignment scores of the jobs mem_flt_chained_seeds poses (meme_kswv.hip): window [rb, rb + tlen) of the text against the tlen x qlen
// bases at reads[qoff]; sc[seed] = score.  The job count is read on the device; max_jobs sizes the launch.
constexpr int MEME_SEEDSW_MAX = 200;    // MEM_SHORT_LEN, src/bwamem.cpp:250: windows are shorter
struct meme_seedsw_job { i64 rb; i64 qoff; int seed; short tlen, qlen; };
int meme_seedsw_launch(meme_ctx* ctx, const meme_seedsw_job* d_jobs, const unsigned long long* d_njobs, i64 max_jobs, int* d_sc, const meme_ext_opt* o);
// the mate-rescue kernels on jobs whose sequences are already in ctx->kswv.ref / qer and whose records are in ctx->kswv.jobs (meme_kswv.hip; the jobs also on the host,
// for the sort into LDS classes); staged = false: meme_kswv_batch_host's own path (sequences and jobs come from the host)
int meme_kswv_run(meme_ctx* ctx, const meme_kswv_job* jobs, int64_t njobs, const uint8_t* ref, int64_t ref_bytes, const uint8_t* qer, int64_t qer_bytes, const meme_bsw_opt* opt,
                  bool staged, meme_kswv_host_result* out);
// the chaining workspace that depends on the read count alone (meme_chain.hip)
int meme_chain_reserve(meme_ctx* ctx, i64 n);
// chains of the batch just seeded, left in HBM (meme_chain.hip); totals[0..1] = chains, chained seeds
int meme_chain_run(meme_ctx* ctx, const meme_contig* contigs, int32_t n_contigs, const meme_chain_opt* opt, i64* totals);

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) {                                                                \
            meme_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return MEME_E_HIP;                                                                 \
        }                                                                                      \
    } while (0)

// ---- device helpers --------------------------------------------------------------------------------
// text position of suffix-array slot i from the 5-byte image: the two aligned dwords around the record
__device__ __forceinline__ u64 load_pos5(const uint8_t* pos5, i64 i) {
    const i64 bo = i * 5;
    const uint32_t* pd = reinterpret_cast<const uint32_t*>(pos5 + (bo & ~3ll));
    const u64 two = (u64)pd[0] | ((u64)pd[1] << 32);
    const u64 v5 = (two >> (8 * (int)(bo & 3))) & 0xffffffffffull;
    return ((v5 & 0xffffffffull) << 8) | (v5 >> 32);
}
// base p of the 2-bit text (DevIndex::pac)
__device__ __forceinline__ int text_base(const u64* pac, i64 p) { return (int)(pac[p >> 5] >> (62 - 2 * (int)(p & 31))) & 3; }
// 32 bases starting at base offset s from a big-endian-within-word 2-bit array
__device__ __forceinline__ u64 extract32(const u64* w, i64 s) {
    i64 k = s >> 5;
    int sh = (int)(s & 31) * 2;
    u64 a = w[k], b = w[k + 1];
    return sh ? (a << sh) | (b >> (64 - sh)) : a;
}
