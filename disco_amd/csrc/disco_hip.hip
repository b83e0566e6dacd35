/*
 * disco_hip.hip — C-ABI implementation (include/disco_hip.h) over the kernels in disco_kernels.h.
 * Built for gfx950 only:  hipcc --offload-arch=gfx950 -O3 -fPIC -shared -o libdisco_hip.so disco_hip.hip
 *
 * Data layout in HBM (n reads, stride S words, T = bucket table size, Eraw = verified overlap hits, E = directed edges):
 *   reads      u64[n][S]      2-bit packed, fixed stride (coalesced row fetches, no offset indirection)
 *   len        u16[n]
 *   bkt        u32[T+1]       CSR bucket table of the end-k-mer index, T = pow2 >= 4n
 *   ent        u64[2n]        8-byte records: key fingerprint | id | minimizer offset | record strand | isSuffix | len
 *   best       u64[n]         containment keys (atomicMin), all-reduced(MIN) across ranks
 *   contained  u8[n]
 *   hits       u64[cap]       raw verified overlap hits, wave-private chunks, rows addressed by row_start/row_cnt
 *   adj_start  u64[n+1], adj u64[E]   adjacency CSR in node order (offset | dst | orient per entry)
 *   flag       u8[E]          bit0 = transitive from this end, bit1 = survives (emitted from this end)
 */
#include <hip/hip_runtime.h>
#include <rocprofiler-sdk-roctx/roctx.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <string>
#include <memory>
#include <thread>
#include <map>
#include <mutex>
#include <queue>
#include <vector>

#include "../../include/disco_hip.h"
#include "../../include/disco_hip_test.h"
#include "../../include/disco_hip_inspect.h"
#include "disco_kernels.h"
#include "disco_dist.h"

#define DROP_LIST_CAP (1u << 20) /* dropped hits edge selection writes down for the twin search (16 MB); more than that: the bitmap search */
#include "disco_chains.h"
#include "disco_text.h"
#include "disco_binrec.h"
#include "disco_gfa.h"
#include "disco_gfa_chains.h"
#include "disco_unitig_reads.h"
#include "disco_partext.h"
#include "disco_ringio.h"
#include "disco_ingest.h"
#include "disco_bgzf.h"
#include "read_filter_tables.h"
#include "disco_comm.h"

static_assert(sizeof(disco_genspec) == sizeof(disco_genspec_abi), "genspec ABI mismatch");

static thread_local std::string g_create_error;

using HClock = std::chrono::steady_clock;
static float ms_since(HClock::time_point t0) { return std::chrono::duration<float, std::milli>(HClock::now() - t0).count(); }

/* phase timers: the public phases (disco_phase_ms) plus one internal slot — the index phase's second bracket (ph_collect adds it to the first) */
#define DISCO_PH_INDEX2 DISCO_PH_COUNT
#define DISCO_PH_SLOTS (DISCO_PH_COUNT + 1)

/* tracing hooks (the reference brackets its functions with CLOCKSTART / CLOCKSTOP, BG/Common.h:71-95): every
 * phase of the path is a named roctx range, so `rocprofv3 --marker-trace --kernel-trace` shows the kernels under the C-ABI call
 * and the phase that launched them; without a tool attached a range costs two calls into an empty library */
struct RoctxRange {
    explicit RoctxRange(const char *name) { (void)roctxRangePushA(name); }
    ~RoctxRange() { (void)roctxRangePop(); }
    RoctxRange(const RoctxRange &) = delete;
    RoctxRange &operator=(const RoctxRange &) = delete;
};
#define DISCO_TRACE(name) RoctxRange roctx_range_(name)

/* host-side loops over tens of millions of results (struct conversion, random reads of the length table) */
template <typename F>
static void parallel_for(u64 n, F f)
{
    unsigned nt = std::thread::hardware_concurrency();
    if (const char *e = getenv("DISCO_HOST_THREADS")) nt = (unsigned)atoi(e);
    nt = std::max(1u, std::min(nt, 16u));
    if (n < (1u << 16) || nt == 1) {
        f((u64)0, n);
        return;
    }
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; t++) th.emplace_back([=]() { f(n * t / nt, n * (t + 1) / nt); });
    for (auto &x : th) x.join();
}


/* What a pass did besides launching kernels, per host thread (= per rank: one thread drives one rank, in-process or not):
 * device allocations and frees that reached the HIP runtime, blocking waits on the device, operations on a communicator. A
 * multi-GPU pass reports them (disco_dist_info): allocations between two collectives of a pass are a hazard when several ranks
 * share a process, and every blocking wait / collective launch is host time on the critical path of an 8-GPU pass. */
struct PassCounters {
    u32 dev_allocs = 0, dev_frees = 0, host_syncs = 0, comm_ops = 0;
};
static thread_local PassCounters tl_pass;
static inline hipError_t counted_stream_sync(hipStream_t s)
{
    tl_pass.host_syncs++;
    return hipStreamSynchronize(s);
}
static inline hipError_t counted_event_sync(hipEvent_t e)
{
    tl_pass.host_syncs++;
    return hipEventSynchronize(e);
}
#define hipStreamSynchronize(s) counted_stream_sync(s)
#define hipEventSynchronize(e) counted_event_sync(e)

/* Arena of a multi-GPU context: ONE device allocation made before the first collective of the first pass; every buffer of the pass
 * is carved out of it (first fit, neighbours coalesced on free: a few hundred calls per pass), so that no hipMalloc / hipFree runs
 * between the collectives of a pass — with one host thread per rank in one process (buildG --gpus N) a device allocation while
 * another rank's RCCL kernels are in flight can serialise against them or deadlock. A request the arena cannot serve falls back to
 * the runtime and is counted (disco_dist_info.device_allocs). */
struct DevArena {
    char *base = nullptr;
    size_t size = 0, used = 0, peak = 0;
    std::map<size_t, size_t> free_at; /* offset -> bytes of every free block */
    bool owns(const void *p) const { return base && (const char *)p >= base && (const char *)p < base + size; }
    void *alloc(size_t bytes)
    {
        bytes = (bytes + 255) & ~(size_t)255;
        for (auto it = free_at.begin(); it != free_at.end(); ++it)
            if (it->second >= bytes) {
                const size_t off = it->first, len = it->second;
                free_at.erase(it);
                if (len > bytes) free_at[off + bytes] = len - bytes;
                live[off] = bytes;
                used += bytes;
                peak = std::max(peak, used);
                return base + off;
            }
        return nullptr;
    }
    void release(void *p)
    {
        const size_t off = (size_t)((char *)p - base);
        auto lv = live.find(off);
        if (lv == live.end()) return;
        size_t start = off, end = off + lv->second;
        used -= lv->second;
        live.erase(lv);
        auto nx = free_at.lower_bound(off); /* the first free block behind the freed one */
        if (nx != free_at.end() && nx->first == end) {
            end += nx->second;
            nx = free_at.erase(nx);
        }
        if (nx != free_at.begin()) {
            auto pv = std::prev(nx);
            if (pv->first + pv->second == start) {
                start = pv->first;
                free_at.erase(pv);
            }
        }
        free_at[start] = end - start;
    }
    std::map<size_t, size_t> live; /* offset -> bytes of every block handed out */
};

/* A device buffer the context owns: the pointer and the elements it was allocated with, which is what release gives back to hbm_bytes.
 * It reads as a plain pointer. Only ensure / ensure_keep / release / adopt / disown (below) change it. The context's members live as
 * long as the context and are released by name (free_graph_state and its like), so DevBuf has no destructor; a function's own buffers
 * are LocalBufs. */
template <typename T>
struct DevBuf {
    T *p = nullptr;
    u64 cap = 0;
    operator T *() const { return p; }
};

struct disco_ctx;
template <typename T>
static void release(disco_ctx *c, DevBuf<T> &b);

/* A device buffer a function (or a short-lived struct) owns: a DevBuf wherever one is taken, released when it leaves its scope, so that
 * CHK / HIPCHK may return from anywhere. release(c, b) before that gives the memory back early (peak memory, the arena's first fit);
 * give / take hand the memory to a member of the context, or borrow a member's for a while, without touching hbm_bytes. */
template <typename T>
struct LocalBuf : DevBuf<T> {
    disco_ctx *const c;
    explicit LocalBuf(disco_ctx *ctx) : c(ctx) {}
    LocalBuf(const LocalBuf &) = delete;
    LocalBuf &operator=(const LocalBuf &) = delete;
    ~LocalBuf() { release(c, *this); }
    void give(DevBuf<T> &to) /* to's own memory is released first */
    {
        release(c, to);
        to = *this;
        DevBuf<T>::operator=(DevBuf<T>());
    }
    void take(DevBuf<T> &from)
    {
        release(c, *this);
        DevBuf<T>::operator=(from);
        from = DevBuf<T>();
    }
};

/* formatted lines that wait on the device to be fetched or written: the files' text one behind the other, the byte range of every file
 * inside it (n_files + 1 offsets), and the bytes in all (0: nothing formatted, whatever d still holds) */
struct TextProduct {
    DevBuf<char> d;
    std::vector<u64> off;
    u64 bytes = 0;
};

struct disco_ctx {
    int device = 0;
    disco_params prm{};
    DevArena arena;
    int k = 0;  /* the reference's k = min_overlap - 1 */
    int ks = 0; /* the seed the index holds: min(k, DISCO_MAX_K) (DISCO_FLAG_SEEDED_KMER; DiscoView::ks) */
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    int n_cu = 256;
    std::string err;
    size_t hbm_bytes = 0, hbm_peak = 0;

    /* reads */
    u64 n = 0;
    int S = 0;
    u64 *d_reads = nullptr; /* what the kernels read: reads_own, or the caller's table (disco_adopt_reads) */
    u16 *d_len = nullptr;   /* ... len_own, or the caller's lengths */
    DevBuf<u64> reads_own;
    DevBuf<u16> len_own;
    bool reads_owned = false;
    std::vector<uint16_t> h_len; /* lazily mirrored for result decoding */
    bool h_len_ok = false;       /* h_len holds the lengths of the current reads */
    std::mutex h_len_mu;         /* disco_ingest_fetch may run on a host thread of its own next to a pass (the one call allowed to):
                                    it and ensure_host_len are the two writers that can meet */
    u64 q_lo = 0, q_hi = 0;
    /* two classes of rows (disco_kernels.h, "two classes of rows"): made by two_class_convert at the first index build over a table whose
     * stride a few long reads forced; c->S is 8 from then on and S_ext what the caller gave (disco_stride_words, disco_download_reads) */
    bool two_class = false;
    bool dist_two_class = false; /* set by a multi-GPU pass around its two_class_convert (round 6) */
    u64 job_n_long = 0;          /* ... reads of more than 256 bases in the whole job, and the longest of the others (dist_validate) */
    u32 job_short_max = 0;
    int S_ext = 0;
    u64 n_long = 0;
    DevBuf<u64> d_full;
    DevBuf<u32> d_ovf, d_long_ids;
    u32 max_len_all = 0; /* longest read of the set (max_len: of the short class) */
    int tailb = 0;
    DevBuf<u32> d_lpos, d_n_list; /* the long reads' candidate rows of the pass (class_take_rows_kernel) */
    DevBuf<uint2> d_linfo;
    DevBuf<ulonglong2> d_lmeta;

    /* index */
    u64 T = 0;
    int bshift = 0;
    DevBuf<u32> d_bkt;
    DevBuf<u64> d_ent;
    DevBuf<ulonglong2> d_rec; /* {key, record}[2n] scratch of the index build; binned build: 2n payloads, then 2n 4-byte keys (index_planes) */
    /* binned build (binned_build_index): decided once per index by index_begin — the count pass then leaves out its bucket atomics and
     * writes the records as planes, and the bucket table is neither cleared nor scanned */
    bool binned_index = false;
    DevBuf<ulonglong2> d_rec2; /* the other side of the partition levels' ping-pong: 2n x 12 bytes in planes (first the grouping's items and theirs) */
    DevBuf<u32> d_binx;        /* segment starts and tile bases of two levels, the tile x bin counts of one */

    /* scan temporaries */
    DevBuf<u64> d_tile;
    u64 *d_total = nullptr;

    /* counters */
    u64 *d_ctr = nullptr;
    u64 *d_wq = nullptr; /* work-queue counter shared by the wave-per-item kernels (one launch at a time) */
    u64 h_ctr[CTR_COUNT] = {0};

    /* probe */
    DevBuf<u64> d_best;
    DevBuf<u64> d_hits;
    u64 hits_used = 0; /* high-water mark of the hit buffer after the probe: what lies behind it is free */
    u64 *d_bump = nullptr;
    DevBuf<u64> d_row_start;
    DevBuf<u32> d_row_cnt;
    DevBuf<u64> d_big_list; /* (list and counts grow together: grow_big_lists) */
    DevBuf<u32> d_big_cnt;
    u32 *d_n_big = nullptr;
    /* minimizer runs of the reads [runs_lo, runs_lo + runs_n) (index_runs_kernel -> probe_runs_kernel): runs_lpr u32 words per read
     * (16: up to 32 runs, reads of up to 128 windows; 32: up to 64 runs, 256 windows), 0 = the index pass left none */
    DevBuf<u32> d_runs;
    u64 runs_lo = 0, runs_n = 0;
    int runs_lpr = 0;
    DevBuf<u64> d_slow_list; /* reads whose run list is unusable (ties, too many runs): probe_kernel<2> */
    u32 *d_n_slow = nullptr;
    u64 big_rows = 0, slow_rows = 0;
    const u64 *d_order = nullptr; /* not owned: a caller's processing order of the query range (plain read ids), or null */
    const u64 *d_order_used = nullptr; /* not owned: what the last probe walked — packed entries (ORDER_MAKE) in d_order_own, or null = file order */
    bool order_external = false;
    DevBuf<u32> d_ocnt, d_okey, d_oslot;
    DevBuf<u64> d_order_own;
    /* the grouping's counting pass ran inside the index pass, for the reads [lo, hi) with 2^bits buckets (d_ocnt holds the counts,
     * d_oslot the slots): the next disco_probe over exactly that range skips its own */
    bool order_counted = false;
    bool order_items = false; /* ... as items for the partition levels (d_rec2; the binned grouping): only disco_build_index can finish it */
    int order_id_bits = 0;    /* (bits of the read id in an item) */
    int order_spare_bits = 0; /* (bits of an item that bucket, length and read id leave) */
    int order_sub_bits = 0;   /* (... and how many of them hold the sub-key, directly below the bucket: ORDER_SUBKEY; 0 = none) */
    int order_sub_limit = ORDER_SUB_MAX; /* (disco_set_order_sub_bits: tests take the sub-key away) */
    /* the big-item lists are sized from counts the producing kernels leave behind (verify: rows beyond ES_CAP; edge selection: nodes
     * beyond TR_CAP) — valid until something else changes the rows: then the counting pass (ensure_big_cap) runs as before */
    bool es_big_counted = false, tr_big_counted = false;
    bool contained_count_pending = false; /* disco_run_graph: n_contained is read with the next counters */
    bool order_ready = false; /* ... and disco_build_index went on to the order itself (d_order_own, for [order_counted_lo, order_counted_hi)): the fill walks it */
    /* contained rows on their way to the host while the pass goes on (disco_mark_contained -> disco_fetch_contained) */
    hipStream_t aux_stream = nullptr;
    hipEvent_t ev_crows = nullptr;
    DevBuf<u32> d_cpos, d_crow_id; /* (d_crow_id / _key / _len grow together) */
    DevBuf<u64> d_crow_key;
    DevBuf<u64> d_tile2; /* scan temporaries of the side stream */
    u64 *d_total2 = nullptr;
    /* pinned, per order (by id, then grouped): keys u64[crows_hcap], ids u32[crows_hcap], lengths u32[crows_hcap] — an allocation of its
     * own, or (crows_in_ring) not owned: the input stage's ring h_ring */
    void *h_crows = nullptr;
    DevBuf<u32> d_crow_len; /* len2 | len1 << 16 of the rows about to leave */
    u64 crows_hcap = 0, crows_n = 0;
    bool crows_pending = false; /* the rows of the CURRENT flags are on their way / in h_crows */
    bool crows_in_ring = false; /* h_crows is the input stage's pinned ring (h_ring), not an allocation of its own */
    DevBuf<u32> d_cgrp_cur, d_cgrp_id; /* the same rows grouped by containing read (disco_fetch_contained_grouped) */
    DevBuf<u64> d_cgrp_key, d_cgrp_big;
    u64 h_cgrp_big = 0;
    bool cgrp_pending = false;
    /* disco_fetch_edges: the compacted edges before they travel (kept across passes) */
    DevBuf<u32> d_fetch_src;
    DevBuf<u64> d_fetch_ent;
    /* input stage on the GPU (disco_ingest_fasta): what disco_ingest_fetch hands to the host afterwards */
    DevBuf<u32> d_rec_of_read;
    std::vector<u64> ingest_id_base, ingest_rec_base; /* per file: first read id, records before the file */
    u64 ingest_n = 0;
    void *h_ring = nullptr; /* pinned: two halves of the text staging ring */
    /* the three texts, each state of its own, so that any may be formatted first: the edge lines of all files, file after file
     * (disco_format_edges), the lines of the contained-read files (disco_format_contained) ... */
    TextProduct text, ctext;
    DevBuf<u8> d_ingest; /* the input stage's own arena (text, record arrays) when the hit buffer is allocated NEXT to it ... */
    std::thread hits_prealloc; /* ... by this thread, while the files travel and the filter runs (settle_hits_prealloc) */
    DevBuf<u64> prealloc; /* (hipMalloc of that thread; settle_hits_prealloc adopts or frees it) */
    u64 prealloc_asked = 0; /* entries that thread was asked for: in hbm_bytes from the call that asks until the thread is joined */
    size_t ring_half = 0;
    hipEvent_t ev_ring[2] = {nullptr, nullptr};
    hipStream_t copy_stream = nullptr; /* disco_upload_reads: the chunks of the host buffer travel here */
    hipEvent_t ev_copied[3] = {nullptr, nullptr, nullptr}, ev_unpacked[3] = {nullptr, nullptr, nullptr};
    bool index_counted = false; /* disco_upload_reads ran the index's count pass behind its copies: disco_build_index starts at the scan */
    u64 order_counted_lo = 0, order_counted_hi = 0;
    int order_counted_bits = 0;
    DevBuf<u32> d_asked; /* multi-GPU flow: one bit per node — its row has been asked for in this pass (tr_request_*_kernel) */
    u64 order_q_lo = 0, order_q_hi = 0;
    DevBuf<ulonglong2> d_meta_ord; /* per-read headers by position in the processing order (probe -> verify) */
    u64 dropped_local = 0;
    ProbeRare h_probe_rare;
    DevBuf<ProbeRare> d_probe_rare;
    u32 max_len = 0, min_len = 0; /* longest / shortest read (validate_reads) */
    bool two_pass_last = false;    /* the last probe verified in two passes */
    bool contained_done = false;   /* multi-GPU pass: the containment exchange already ran between the two verify passes */

    /* containment */
    DevBuf<u8> d_contained;
    DevBuf<u64> d_cbits; /* one bit per read */
    DevBuf<u64> d_dropbits; /* one bit per read: its edge selection dropped a verified hit; valid for reads [drop_lo, drop_hi) */
    DevBuf<u64> d_drop_node, d_drop_key; /* exact overlaps: the dropped hits themselves (EdgeSelArgs.drop_node), DROP_LIST_CAP items */
    u64 n_drop_items = 0;                              /* how many the last selection recorded (or would have: > DROP_LIST_CAP = list useless) */
    u64 drop_lo = 0, drop_hi = 0;
    u64 n_contained = 0;

    /* edges */
    DevBuf<u64> d_adj_ref; /* [n] position | degree << 40 */
    u64 *d_adj = nullptr;     /* not owned: the entries — the hit buffer itself (single GPU) or d_adj_own (imported / merged, node-ordered) */
    DevBuf<u64> d_adj_own; /* kept across passes: re-allocating GBs every pass costs more than the kernels */
    DevBuf<u64> d_adj_spare; /* the rebuilding merge writes here and swaps: its 9 GB at 50 M reads are not allocated and freed per pass */
    DevBuf<u64> d_start_tmp; /* [n+1] scan scratch of export / import */
    u64 adj_total = 0; /* directed edges the context currently addresses */
    bool flags_pending = false; /* sharded flow: gathered flag bytes wait to be OR-ed into the entries */
    bool adj_imported = false;
    u64 adj_span = 0;          /* size of the position space of d_adj in the sharded flow (compact: adj_total, padded: world*max) */
    bool half_complete = false; /* half/hcnt hold the survivor lists of ALL nodes */
    bool half_selfdel = false;  /* the lists carry their own end (disco_survivor.h) and hcnt was not written: the whole-table pass of one GPU */
    DevBuf<u32> d_extra_cnt;
    DevBuf<u64> d_extra_node, d_extra_key; /* (grow together) */
    u32 *d_n_extra = nullptr;
    u32 n_extra = 0;
    u64 asym_local = 0;
    u64 dropped = 0; /* hits edge selection dropped in the local query range (0 => the selected edges are symmetric) */

    /* reduction */
    DevBuf<u64> d_half; /* [n][HALF_CAP] */
    DevBuf<u32> d_hcnt; /* [n] */
    bool use_half = false;
    DevBuf<u64> d_wide; /* nodes with more than HALF_CAP surviving edges */
    DevBuf<u32> d_n_wide;
    u32 n_wide = 0;
    DevBuf<u8> d_out_valid; /* (with d_out_pos: sized together) */
    DevBuf<u64> d_out_pos;
    u64 *h_stage = nullptr; /* pinned: two halves of {sources, entries} for the chunked copy-out of disco_fetch_edges */
    hipEvent_t ev_stage[2] = {nullptr, nullptr};
    /* chain contraction (disco_contract_chains): composite edges, their links, absorbed flag per edge in fetch order */
    DevBuf<ChainEdgeOut> d_ch_comp;
    DevBuf<ChainLinkOut> d_ch_links;
    DevBuf<u8> d_ch_dead;
    u64 ch_comp_n = 0, ch_links_n = 0, ch_edges_n = 0;
    bool ch_ready = false;
    /* ... and what the host pass needs of it (disco_fetch_chain_residue / _first_edges): the edges no composite took, by fetch-order
     * position and by slot, and the position of the edge behind every composite's first link */
    DevBuf<u64> d_ch_first, d_ch_res_pos, d_ch_res_slot;
    u64 ch_res_n = 0;
    bool ch_resident = false; /* contracted from the emission's slots (disco_contract_chains), which still hold the records */
    TextProduct ptext; /* ... and the lines of the ParSimpleEdges files (disco_format_par_simple) */
    /* the records of the binary side output (disco_prepare_*_records, disco_binrec.h): what a prepare call uploaded or grouped, kept until
     * the next pass; the records themselves exist one piece at a time (d_rec_piece: two buffers of rec_piece_cap records) */
    DevBuf<u16> d_rec_efile, d_rec_subs;
    DevBuf<u64> d_rec_efindex, d_rec_cfindex;
    DevBuf<u64> d_rec_cword; /* the contained rows, grouped and sorted (group_contained_rows) */
    DevBuf<u32> d_rec_csup;
    bool rec_e_ready = false, rec_e_has_file = false, rec_e_has_findex = false, rec_e_has_subs = false;
    bool rec_c_ready = false, rec_c_has_findex = false;
    u32 rec_e_files = 0, rec_c_files = 0;
    u64 rec_c_n = 0;
    DevBuf<u8> d_rec_piece[2];
    u64 rec_piece = 0; /* records per piece; 0: what a ring half holds (disco_set_record_piece: tests) */
    DevBuf<u64> d_out_src, d_out_ent; /* (grow together) */
    u64 out_used = 0; /* chunk slots written by the emission (survivors + ~0 tails) */
    bool out_dense = false; /* the last emission wrote no tails: slot i is edge i, out_used == n_out, d_out_valid / d_out_pos are not there */
    u64 n_out = 0;

    /* live kernel timing (HIP events on the stream the kernels are launched on) */
    hipEvent_t ev0[DISCO_PH_SLOTS] = {nullptr}, ev1[DISCO_PH_SLOTS] = {nullptr};
    bool ev_pending[DISCO_PH_SLOTS] = {false};
    float ph_ms[DISCO_PH_SLOTS] = {0};

    int phase = 0; /* 0 none, 1 reads, 2 index, 3 probe, 4 contained, 5 edges selected, 6 symmetrized, 7 marked, 8 emitted */

    /* multi-GPU flow (disco_comm_* / disco_dist_*): one context per rank */
    DiscoComm *comm = nullptr;
    DiscoComm *comm_bulk = nullptr;   /* a second communicator for the all-gather of the reads: it runs on bulk_stream while the */
    hipStream_t bulk_stream = nullptr; /* index is built and the own reads are probed (only verify needs the other ranks' rows)  */
    hipEvent_t ev_bulk = nullptr;
    bool wait_bulk_before_verify = false;
    u64 per = 0;        /* nodes per rank: ceil(n / world) rounded up to a multiple of 64 */
    u64 n_alloc = 0;    /* rows of the per-read tables (n on one GPU, world * per in the multi-GPU flow) */
    bool part_index = false;   /* the current multi-GPU pass keeps the index partitioned (DISCO_DIST_KEEP_INDEX_PARTITIONED) */
    u64 part_blo = 0, part_bhi = 0, part_nrec = 0; /* this rank's bucket range and records */
    DevBuf<u64> d_pq_start; /* scan scratch of the lookup exchange */
    bool dist_reads = false;   /* the read table was set through disco_dist_*: rows [q_lo, q_hi) are this rank's */
    bool dist_active = false;  /* the current pass is a multi-GPU pass in the regular regime (emission judges local pairs only) */
    DevBuf<u64> d_route;    /* [2 * DIST_MAX_WORLD] counters / cursors of the routing kernels */
    DevBuf<ulonglong2> d_x16a, d_x16b; /* 16-byte items: send (partitioned) / receive */
    DevBuf<u32> d_req_flat, d_req_s, d_req_r; /* row requests: flat list, partitioned, received */
    DevBuf<u32> d_rdeg_s, d_rdeg_r, d_rdata_s; /* responses: degrees out / back, entries out */
    DevBuf<u64> d_rpos;
    DevBuf<u32> d_nadj32_own; /* rows fetched from other ranks as they arrive (4-byte entries), before rows_place_kernel puts them behind the own rows */
    u64 nadj_used = 0; /* entries of fetched rows behind the own rows so far */
    DevBuf<u32> d_deg_tmp;
    DevBuf<u64> d_list_n; /* length of the flat list being built */
    DevBuf<u64> d_dense; /* the job's reads at W words per row, for the all-gather (rows of the table are padded to 64 bytes) */
    ulonglong2 *d_push_r = nullptr; /* not owned: received half-edge pushes (d_x16b while a pass is in flight) */
    u64 n_push_r = 0;
    /* ranks own loci: the reads — graph nodes — of a pass are dealt to the ranks by their read-level minimizer;
     * [home_lo, home_hi) is the id range the rank's reads arrived in (and the range whose containment flags it fixes). While such a pass
     * runs, q_lo / q_hi are POSITIONS in the rank's own list: [0, n_own) of d_order_own. */
    bool loci = false;
    bool runs_by_pos = false; /* d_runs is indexed by position in the processing order, not by read id */
    DevBuf<u8> d_otab;     /* [n_alloc] owner of every read */
    DevBuf<u32> d_own_ids; /* scratch: the own reads before they are grouped */
    u64 n_own = 0;
    u64 home_lo = 0, home_hi = 0;
    u64 home_probes = 0; /* sum of len - k over the home range */
    /* the containment keys' reduce-scatter runs behind the pass on the second communicator (dist_mark_contained): whoever touches best[]
     * next waits for ev_keys */
    DevBuf<u64> d_cb_all; /* the ranks' "has a key" bitmaps, rank after rank */
    hipEvent_t ev_keys = nullptr, ev_keys_go = nullptr;
    bool keys_pending = false;
    disco_dist_info dinfo{};
    /* wait behind every all-to-all so that dinfo.ms shows the exchange and not its issue: DISCO_DIST_TIME_EXCHANGES=1, and — first contact
     *  — the FIRST pass of a context over RCCL with more than one rank (the pass a bench warms up with, the pass a watchdog
     * report is about: a stall then names the exchange it sits in); DISCO_DIST_NO_FIRST_CONTACT=1 takes that away */
    bool time_exchanges = false;
    unsigned dist_passes = 0;
};

/* ---------------------------------------------------------------------------------------------------------------- */
static int fail(disco_ctx *c, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    else g_create_error = buf;
    return code;
}

#define HIPCHK(c, call)                                                                                          \
    do {                                                                                                         \
        hipError_t e_ = (call);                                                                                  \
        if (e_ != hipSuccess) return fail((c), e_ == hipErrorOutOfMemory ? DISCO_E_NOMEM : DISCO_E_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

#define CHK(expr)                    \
    do {                             \
        int rc_ = (expr);            \
        if (rc_ != DISCO_OK) return rc_; \
    } while (0)

static void ph_begin(disco_ctx *c, int id)
{
    (void)hipEventRecord(c->ev0[id], c->stream);
}
static void ph_end(disco_ctx *c, int id)
{
    (void)hipEventRecord(c->ev1[id], c->stream);
    c->ev_pending[id] = true;
}
/* call after the stream has been synchronised */
static void ph_collect(disco_ctx *c)
{
    for (int i = 0; i < DISCO_PH_SLOTS; i++)
        if (c->ev_pending[i]) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, c->ev0[i], c->ev1[i]) == hipSuccess) c->ph_ms[i] = ms;
            c->ev_pending[i] = false;
            if (i == DISCO_PH_INDEX) c->ph_ms[DISCO_PH_INDEX2] = 0; /* (a new index phase: its second bracket, if it has one, is collected below) */
        }
    /* the index phase in two brackets (the grouping sits between its count pass and its fill): reported as one */
    if (c->ph_ms[DISCO_PH_INDEX2] > 0) {
        c->ph_ms[DISCO_PH_INDEX] += c->ph_ms[DISCO_PH_INDEX2];
        c->ph_ms[DISCO_PH_INDEX2] = 0;
    }
}

template <typename T>
static int dev_alloc(disco_ctx *c, T **p, size_t count)
{
    size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    if (c->arena.base) {
        if (void *q = c->arena.alloc(bytes)) {
            *p = (T *)q;
            c->hbm_bytes += bytes;
            c->hbm_peak = std::max(c->hbm_peak, c->hbm_bytes);
            return DISCO_OK;
        }
    }
    tl_pass.dev_allocs++;
    HIPCHK(c, hipMalloc((void **)p, bytes));
    c->hbm_bytes += bytes;
    c->hbm_peak = std::max(c->hbm_peak, c->hbm_bytes);
    return DISCO_OK;
}

template <typename T>
static void dev_free(disco_ctx *c, T **p, size_t count)
{
    if (*p) {
        if (c->arena.owns(*p)) c->arena.release(*p);
        else {
            tl_pass.dev_frees++;
            (void)hipFree(*p);
        }
        c->hbm_bytes -= std::max<size_t>(count, 1) * sizeof(T);
        *p = nullptr;
    }
}

template <typename T>
static void release(disco_ctx *c, DevBuf<T> &b)
{
    dev_free(c, &b.p, b.cap);
    b.cap = 0;
}

/* grow-only: reallocate when the need exceeds the capacity (steady-state passes allocate nothing) */
template <typename T>
static int ensure(disco_ctx *c, DevBuf<T> &b, u64 need)
{
    if (b.p && need <= b.cap) return DISCO_OK;
    release(c, b);
    CHK(dev_alloc(c, &b.p, need));
    b.cap = std::max<u64>(need, 1);
    return DISCO_OK;
}

/* buffers that grow together (the kernels take one capacity for all of them): when any holds fewer than `need` elements, all are freed
 * and then allocated with `size` elements each, in order (the arena's first fit sees the frees before the allocations); a failure leaves
 * none of them allocated, so the next call allocates them all again */
template <typename... T>
static int ensure_group(disco_ctx *c, u64 need, u64 size, DevBuf<T> &...b)
{
    if (((need <= b.cap) && ...)) return DISCO_OK;
    (release(c, b), ...);
    int rc = DISCO_OK;
    ((rc = rc == DISCO_OK ? ensure(c, b, size) : rc), ...);
    if (rc != DISCO_OK) (release(c, b), ...);
    return rc;
}

/* b moves to a new allocation of ncap elements that starts with its first `used` ones */
template <typename T>
static int move_keep(disco_ctx *c, DevBuf<T> &b, u64 ncap, u64 used)
{
    LocalBuf<T> q(c);
    CHK(ensure(c, q, ncap));
    if (b.p && used) HIPCHK(c, hipMemcpyAsync(q.p, b.p, used * sizeof(T), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    q.give(b);
    return DISCO_OK;
}

/* grow-only buffer that keeps its first `used` elements */
template <typename T>
static int ensure_keep(disco_ctx *c, DevBuf<T> &b, u64 need, u64 used)
{
    if (b.p && need <= b.cap) return DISCO_OK;
    return move_keep(c, b, need + need / 8, used);
}

/* hand-overs: b (empty) takes memory allocated outside dev_alloc, counted from now on; disown gives b's memory up without freeing it */
template <typename T>
static void adopt(disco_ctx *c, DevBuf<T> &b, DevBuf<T> from)
{
    b = from;
    c->hbm_bytes += b.cap * sizeof(T);
}

template <typename T>
static T *disown(disco_ctx *c, DevBuf<T> &b)
{
    T *p = b.p;
    c->hbm_bytes -= b.cap * sizeof(T);
    b = DevBuf<T>();
    return p;
}

static DiscoView view(const disco_ctx *c)
{
    DiscoView v;
    v.reads = c->d_reads;
    v.len = c->d_len;
    v.n = c->n;
    v.S = c->S;
    v.k = c->k;
    v.ks = c->ks;
    v.m = disco_minimizer_len(c->ks);
    if (const char *e = getenv("DISCO_MINIMIZER_LEN")) { /* tuning knob: odd, <= min(k, 23), k - m <= 63 */
        const int m = atoi(e);
        if (m >= 1 && (m & 1) && m <= v.m && c->ks - m <= 63) v.m = m;
    }
    v.bkt = c->d_bkt;
    v.ent = c->d_ent;
    v.bshift = c->bshift;
    v.q_lo = c->q_lo;
    v.q_hi = c->q_hi;
    v.ctr = c->d_ctr;
    v.wq = c->d_wq;
    v.full = c->two_class ? c->d_full : nullptr;
    v.ovf = c->two_class ? c->d_ovf : nullptr;
    v.long_ids = c->two_class ? c->d_long_ids : nullptr;
    v.n_long = c->two_class ? (u32)c->n_long : 0u;
    v.SL = c->two_class ? c->S_ext : 0;
    v.tailb = c->two_class ? c->tailb : 0;
    return v;
}

/* the nodes the context works on as an OwnSet: the query range, or — inside a multi-GPU pass whose ranks own loci — the own list */
static OwnSet own_set(const disco_ctx *c)
{
    OwnSet o;
    o.otab = c->loci ? c->d_otab : nullptr;
    o.me = c->comm ? (u32)c->comm->rank : 0u;
    o.lo = c->q_lo;
    o.hi = c->q_hi;
    o.list = c->loci ? c->d_order_own : nullptr;
    o.n_own = c->loci ? c->n_own : 0;
    o.ids = c->loci ? c->d_own_ids : nullptr;
    return o;
}

/* best[] of the home range is final only when the reduce-scatter that runs behind the pass is through: the context's stream waits for it */
static int settle_keys(disco_ctx *c)
{
    if (c->keys_pending) {
        c->keys_pending = false;
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_keys, 0));
    }
    return DISCO_OK;
}

static int env_int(const char *name, int dflt)
{
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
}

static int wave_grid(const disco_ctx *c, u64 items, int per_cu = 24)
{
    u64 g = (u64)c->n_cu * per_cu;
    if (items < g) g = items;
    return (int)std::max<u64>(g, 1);
}

/* grid for a work-queue kernel: every workgroup that can be resident (the queue balances the load), zeroes the queue */
template <typename K>
static int wq_grid(disco_ctx *c, K kernel, u64 items, const char *env, int cap = 32)
{
    (void)hipMemsetAsync(c->d_wq, 0, sizeof(u64) * WQ_WORDS, c->stream);
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 64, 0) != hipSuccess || per_cu <= 0) per_cu = 16;
    if (per_cu > cap) per_cu = cap;
    per_cu = env_int(env, per_cu);
    u64 g = (u64)c->n_cu * per_cu;
    const u64 chunks = (items + WQ_CHUNK - 1) / WQ_CHUNK;
    if (chunks < g) g = chunks;
    return (int)std::max<u64>(g, 1);
}

/* a work-queue kernel sized and launched from ONE pointer (these kernels are tuned by resident blocks per CU: a grid sized from one
 * instantiation and launched with another is a silent slowdown). Where the grid is needed first (disco_probe sizes its hit buffer from
 * it): wq_grid with the pointer, and the same pointer to the launch */
template <typename K, typename... A>
static void wq_launch(disco_ctx *c, K kernel, u64 items, const char *env, int cap, A... args)
{
    const int g = wq_grid(c, kernel, items, env, cap);
    hipLaunchKernelGGL(kernel, dim3(g), dim3(64), 0, c->stream, args...);
}

static int flat_grid(const disco_ctx *c, u64 items, int block = 256)
{
    u64 g = (items + block - 1) / block;
    u64 cap = (u64)c->n_cu * 16;
    return (int)std::max<u64>(std::min(g, cap), 1);
}

static int read_counters(disco_ctx *c)
{
    HIPCHK(c, hipMemcpyAsync(c->h_ctr, c->d_ctr, sizeof(c->h_ctr), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DISCO_OK;
}

static int zero_counter(disco_ctx *c, int idx)
{
    HIPCHK(c, hipMemsetAsync(c->d_ctr + idx, 0, sizeof(u64), c->stream));
    return DISCO_OK;
}

/* exclusive scan of in[0..n) into out[0..n) (+ out[n] = total when write_total); returns total through *total_host
 * when non-null (this synchronises the stream) */
template <typename InT, typename OutT>
static int scan_exclusive_on(disco_ctx *c, hipStream_t st, DevBuf<u64> &tile, u64 *total, const InT *in, u64 n, OutT *out, bool write_total, u64 *total_host)
{
    u64 nt = (n + SCAN_TILE - 1) / SCAN_TILE;
    if (nt == 0) nt = 1;
    CHK(ensure(c, tile, nt));
    hipLaunchKernelGGL((scan_tile_sums_kernel<InT>), dim3((unsigned)nt), dim3(SCAN_BLOCK), 0, st, in, n, tile.p);
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(1024), 0, st, tile.p, nt, total);
    hipLaunchKernelGGL((scan_apply_kernel<InT, OutT>), dim3((unsigned)nt), dim3(SCAN_BLOCK), 0, st, in, n, tile.p, out);
    if (write_total) hipLaunchKernelGGL((scan_write_total_kernel<OutT>), dim3(1), dim3(1), 0, st, total, out + n);
    HIPCHK(c, hipGetLastError());
    if (total_host) {
        HIPCHK(c, hipMemcpyAsync(total_host, total, sizeof(u64), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
    }
    return DISCO_OK;
}

template <typename InT, typename OutT>
static int scan_exclusive(disco_ctx *c, const InT *in, u64 n, OutT *out, bool write_total, u64 *total_host)
{
    return scan_exclusive_on<InT, OutT>(c, c->stream, c->d_tile, c->d_total, in, n, out, write_total, total_host);
}

/* what disco_prepare_edge_records / disco_prepare_contained_records left belongs to the pass that made the edges / the contained flags:
 * the phases that make new ones take it away (the piece buffers stay: they are sized by the piece, not by the pass) */
static void drop_edge_records(disco_ctx *c)
{
    c->rec_e_ready = false;
    release(c, c->d_rec_efile);
    release(c, c->d_rec_subs);
    release(c, c->d_rec_efindex);
}
static void drop_contained_records(disco_ctx *c)
{
    c->rec_c_ready = false;
    c->rec_c_n = 0;
    release(c, c->d_rec_cword);
    release(c, c->d_rec_csup);
    release(c, c->d_rec_cfindex);
}

static void free_graph_state(disco_ctx *c)
{
    drop_edge_records(c);
    drop_contained_records(c);
    release(c, c->d_rec_piece[0]);
    release(c, c->d_rec_piece[1]);
    /* a key exchange that still runs behind a pass (second communicator, bulk_stream) reads and writes best[]: it is through before the
     * buffer goes back to the arena — a pass that failed after the exchange was issued, or new reads right after a pass, used to free
     * it under the collective */
    if (c->keys_pending) {
        c->keys_pending = false;
        if (c->ev_keys) (void)hipEventSynchronize(c->ev_keys);
    }
    release(c, c->d_bkt);
    release(c, c->d_ent);
    release(c, c->d_rec);
    release(c, c->d_rec2);
    release(c, c->d_binx);
    release(c, c->d_best);
    release(c, c->d_hits);
    release(c, c->d_row_start);
    release(c, c->d_row_cnt);
    release(c, c->d_big_list);
    release(c, c->d_big_cnt);
    release(c, c->d_slow_list);
    release(c, c->d_runs);
    c->runs_n = 0;
    c->runs_lpr = 0;
    release(c, c->d_contained);
    release(c, c->d_cbits);
    release(c, c->d_dropbits);
    release(c, c->d_drop_node);
    release(c, c->d_drop_key);
    release(c, c->d_adj_ref);
    release(c, c->d_adj_own);
    release(c, c->d_adj_spare);
    release(c, c->d_start_tmp);
    release(c, c->d_ocnt);
    release(c, c->d_okey);
    release(c, c->d_meta_ord);
    release(c, c->d_asked);
    release(c, c->d_oslot);
    release(c, c->d_order_own);
    c->d_order_used = nullptr;
    c->d_adj = nullptr;
    release(c, c->d_extra_cnt);
    release(c, c->d_extra_node);
    release(c, c->d_extra_key);
    release(c, c->d_half);
    release(c, c->d_hcnt);
    release(c, c->d_wide);
    release(c, c->d_n_wide);
    c->adj_total = 0;
    release(c, c->d_out_valid);
    release(c, c->d_ch_comp);
    release(c, c->d_ch_links);
    release(c, c->d_ch_dead);
    release(c, c->d_ch_first);
    release(c, c->d_ch_res_pos);
    release(c, c->d_ch_res_slot);
    c->ch_res_n = 0;
    release(c, c->ptext.d);
    c->ptext.bytes = 0;
    c->ptext.off.clear();
    release(c, c->text.d);
    c->text.bytes = 0;
    release(c, c->ctext.d);
    c->ctext.bytes = 0;
    c->ctext.off.clear();
    c->ch_ready = false;
    release(c, c->d_out_pos);
    release(c, c->d_out_src);
    release(c, c->d_out_ent);
    c->n_out = c->out_used = 0;
    c->flags_pending = false;
    c->adj_imported = false;
    c->T = 0;
    release(c, c->d_x16a);
    release(c, c->d_x16b);
    release(c, c->d_req_flat);
    release(c, c->d_req_s);
    release(c, c->d_req_r);
    release(c, c->d_rdeg_s);
    release(c, c->d_rdeg_r);
    release(c, c->d_rdata_s);
    release(c, c->d_rpos);
    release(c, c->d_nadj32_own);
    release(c, c->d_deg_tmp);
    release(c, c->d_dense);
    release(c, c->d_pq_start);
    c->nadj_used = 0;
    c->d_push_r = nullptr;
    c->n_push_r = 0;
    release(c, c->d_cb_all);
    release(c, c->d_otab);
    release(c, c->d_own_ids);
    c->n_own = 0;
    c->loci = c->runs_by_pos = false;
}

/* the buffers of the long class (two classes of rows) — whatever of them exists: a failed two_class_alloc leaves some behind with
 * two_class still false, and the next table must not find a d_ovf sized for this one */
static void free_long_class(disco_ctx *c)
{
    release(c, c->d_full);
    release(c, c->d_ovf);
    release(c, c->d_long_ids);
    release(c, c->d_lpos);
    release(c, c->d_lmeta);
    release(c, c->d_linfo);
    release(c, c->d_n_list);
    c->two_class = false;
    c->n_long = 0;
    c->S_ext = 0;
    c->tailb = 0;
}

static void free_reads(disco_ctx *c)
{
    release(c, c->reads_own);
    release(c, c->len_own);
    free_long_class(c);
    c->d_reads = nullptr;
    c->d_len = nullptr;
    c->reads_owned = false;
    c->h_len.clear();
    c->n = 0;
}

/* a read table of the context's own: rows of `words` words in all, n_len lengths */
static int alloc_reads(disco_ctx *c, u64 words, u64 n_len)
{
    CHK(ensure(c, c->reads_own, words));
    c->d_reads = c->reads_own;
    CHK(ensure(c, c->len_own, n_len));
    c->d_len = c->len_own;
    return DISCO_OK;
}

/* the twin search's extras lists (node and key arrays grow together): the capacity both have, as the kernels take it */
static u32 extra_cap(const disco_ctx *c) { return (u32)std::min<u64>(std::min(c->d_extra_node.cap, c->d_extra_key.cap), 0xFFFFFFFFull); }

/* the big-item lists (rows / nodes beyond the LDS capacities; fewer than 2^32): list and counts grow together */
static int grow_big_lists(disco_ctx *c, u64 need) { return ensure_group(c, need, need, c->d_big_list, c->d_big_cnt); }

/* the count pass of the index build over the reads [lo, hi): with the minimizer runs for probe_runs_kernel where the shape of the job
 * allows them — a window of 17 m-mers (min-overlap 40, the default), 64-byte rows (reads up to 256 bases, so a read has at most 256
 * windows), and memory for 64 / 128 bytes per read (DISCO_RUNS_MAX_GB, default 16: beyond that — config 5's 2 x 10^8 reads on ONE
 * GPU — the buffer would crowd the hit buffer out of the 288 GB) — otherwise index_count_kernel and the wave-per-read probe_kernel. */
/* does disco_probe group a query range of nq reads itself, and into how many buckets (about one per read: a group has ~13 reads at
 * 30x, few groups share a bucket) */
static bool own_order_wanted(const disco_ctx *c, u64 nq, int *bits)
{
    const u64 order_min = getenv("DISCO_ORDER_MIN_READS") ? (u64)atoll(getenv("DISCO_ORDER_MIN_READS")) : 4096; /* tests: 1 */
    int b = 16;
    while (b < 27 && (1ull << b) < nq) ++b;
    if (const char *e = getenv("DISCO_ORDER_BITS")) b = std::min(std::max(atoi(e), 12), 26); /* tests: two partition levels on a small set; dozens of reads per bucket */
    *bits = b;
    return !c->order_external && !getenv("DISCO_NO_ORDER") && nq >= order_min && nq > 0;
}

/* the count pass in two steps so that it can run chunk by chunk behind an upload (disco_upload_reads): index_count_plan fixes, for the
 * whole range [lo, hi), whether the minimizer runs and the grouping's counting pass ride along and sizes their buffers;
 * index_count_chunk launches the kernel over a sub-range. */
struct IndexCountPlan {
    u64 lo = 0, hi = 0;
    int lpr = 0, nf = 0;
    u32 *ocnt = nullptr, *oslot = nullptr;
    u64 *oitem = nullptr; /* the binned grouping: an item per read instead of a count and a slot */
    u32 oidbits = 0;
    u32 oshift = 0;
    u32 osub = 0; /* the sub-key of an item (ORDER_SUBKEY): its bits << 24 | its multiplier; 0 = none */
    const u64 *list = nullptr; /* ranks own loci: position x of [lo, hi) stands for read ORDER_ID(list[x]) (records, runs, slots by position) */
};

/* the window lengths index_runs_kernel has an instantiation of their own for (a block of NF order words in registers): the reference's
 * default min-overlap 30 (NF 7), 35, BASELINE's 40 (NF 17), 45, 50 */
static bool runs_nf_built(int nf, int m) { return (nf == 7 || nf == 12 || nf == 17 || nf == 22 || nf == 27) && m == RUNS_M; }

/* 32-bit words of minimizer runs per read for a table of 64-byte rows whose longest read has max_len bases, or 0: no runs */
static int runs_lpr_for(const disco_ctx *c, int nf, u32 max_len, u64 nloc)
{
    int lpr = 0;
    /* round 6: every other window of 2 .. 64 m-mers — any min-overlap up to 95, k above 64 and minimizers of up to 31 bases included —
     * takes the instantiation with a run-time window length (DISCO_NO_GENERIC_RUNS=1: round 2's probe for those, as before) */
    const int m = view(c).m;
    const bool nf_built = runs_nf_built(nf, m);
    const bool nf_generic = nf >= 2 && nf <= 64 && m > 16 && m <= 31 && !getenv("DISCO_NO_GENERIC_RUNS");
    if ((nf_built || nf_generic) && max_len > (u32)c->ks && !getenv("DISCO_NO_RUNS")) {
        const u32 maxwin = max_len - (u32)c->ks; /* (the seed's windows) */
        /* a read of W windows has about 2 W / (NF + 1) runs: 32 entries where that stays below 20 (room for the spread), else 64 */
        const u32 expect = 2u * maxwin / (u32)(nf + 1);
        lpr = maxwin <= 256 ? (maxwin <= 128 && expect <= 20 ? 16 : (expect <= 44 ? 32 : 0)) : 0;
        const double max_gb = getenv("DISCO_RUNS_MAX_GB") ? atof(getenv("DISCO_RUNS_MAX_GB")) : 16.0;
        if ((double)nloc * lpr * 4.0 > max_gb * 1e9) lpr = 0;
    }
    return lpr;
}

/* may a table of stride S (words) with n_long reads of more than 256 bases — the others at most short_max — go to two classes of rows? */
/* will_own: the caller is about to replace the table by one the context owns (an upload, the input stage) — the flag itself is only
 * set once the old table has been released and the new buffers exist (a table adopted from the caller must never be freed or kept) */
static bool two_class_ok(const disco_ctx *c, int S, u64 n, u64 n_long, u32 short_max, bool will_own = false)
{
    /* (a context with a communicator: only where its pass asks for it — dist_two_class, after the gather of the reads, over id ranges) */
    if (((c->comm || c->dist_reads) && !c->dist_two_class) || !(c->reads_owned || will_own) || c->prm.max_substitutions || getenv("DISCO_NO_TWO_CLASS")) return false;
    if (S <= VERIFY_SW || n_long == 0 || n_long * (u64)env_int("DISCO_TWO_CLASS_ONE_IN", 5) > n || n + n_long >= (1ull << 31)) return false;
    /* the short class takes the paths of a pure short set (minimizer runs, flat verify); the long one the lists those paths keep */
    return runs_lpr_for(c, c->ks - view(c).m + 1, short_max, n) != 0;
}

/* the long class's buffers for a table of n_long long reads of stride Sx whose short class has reads of up to short_max bases; the rows
 * themselves (d_reads: [n + n_long][8]) are the caller's */
static int two_class_alloc(disco_ctx *c, u64 n_long, int Sx, u32 short_max)
{
    /* (the sizes first: free_long_class accounts with them, also for what a failure below leaves behind) */
    c->n_long = n_long;
    c->S_ext = Sx;
    int rc = ensure(c, c->d_ovf, c->n_alloc);
    if (rc == DISCO_OK) rc = ensure(c, c->d_full, n_long * (u64)Sx);
    if (rc == DISCO_OK) rc = ensure(c, c->d_long_ids, n_long);
    if (rc == DISCO_OK) rc = ensure(c, c->d_lpos, n_long);
    if (rc == DISCO_OK) rc = ensure(c, c->d_lmeta, n_long);
    if (rc == DISCO_OK) rc = ensure(c, c->d_linfo, n_long);
    if (rc == DISCO_OK) rc = ensure(c, c->d_n_list, 1);
    if (rc != DISCO_OK) {
        free_long_class(c);
        return rc;
    }
    c->S = VERIFY_SW;
    c->tailb = short_max <= 160 ? 160 : 256; /* what the staged compare of the short class moves per row (verify_flat_kernel<5 / 8>) */
    c->two_class = true;
    if (getenv("DISCO_VERBOSE"))
        fprintf(stderr, "[disco] two classes of rows: %llu of %llu reads are longer than 256 bases, the others up to %u: 64-byte rows + %d-word rows for those\n",
                (unsigned long long)n_long, (unsigned long long)c->n, short_max, Sx);
    return DISCO_OK;
}

/* (list: the own list of a rank that owns loci, [lo, hi) = its positions — it IS the processing order: no grouping to count) */
/* does the grouping of the whole range go through the partition levels (binned_build_order)? Where the ordered path finishes the
 * grouping inside disco_build_index: one class of rows, no list. DISCO_NO_BINNED_ORDER=1: the counting atomics, the scan of the counter
 * table and the scatter, as before. An item is ONE word — bucket | length | read id (ORDER_ITEM) — so the three must fit: 26 + 8 + 26 bits
 * at 5 x 10^7 reads of 150 bases, and up to 2^28 reads of up to 256 bases; what does not fit keeps the counting form. The items and the
 * other side of their ping-pong are two stretches of d_rec2, which is idle until the record build starts: where it cannot be had, the
 * old path. *id_bits: bits of the read id in an item */
static bool binned_order_wanted(disco_ctx *c, u64 n, int obits, int *id_bits)
{
    if (getenv("DISCO_NO_BINNED_ORDER") || getenv("DISCO_NO_ORDERED_FILL") || c->two_class || n != c->n || n >= 0xFFFF0000ull) return false;
    /* size policy: the chain is nine launches where the old path has five — index + order at 1 M reads 0.31 ms against 0.26 on the old path,
     * at 3 M 0.77 against 0.84, at 10 M 2.33 against 2.65 (profiles/binned_order_ab.txt): from 2^21 reads up (tests: 1) */
    const u64 binned_min = getenv("DISCO_BINNED_ORDER_MIN_READS") ? (u64)atoll(getenv("DISCO_BINNED_ORDER_MIN_READS")) : (1ull << 21);
    if (n < binned_min) return false;
    int idb = 1, lenb = 1;
    while ((1ull << idb) < n) ++idb;
    while ((1u << lenb) <= c->max_len) ++lenb;
    if (obits + lenb + idb > 64) return false;
    if (ensure(c, c->d_rec2, n) != DISCO_OK) { /* (n two-word records = 2 n items) */
        (void)hipGetLastError();
        c->err.clear();
        return false;
    }
    *id_bits = idb;
    c->order_spare_bits = 64 - (obits + lenb + idb);
    return true;
}

static int index_count_plan(disco_ctx *c, const DiscoView &v, u64 lo, u64 hi, IndexCountPlan *pl, const u64 *list = nullptr)
{
    const u64 nloc = hi - lo;
    *pl = IndexCountPlan();
    pl->lo = lo;
    pl->hi = hi;
    pl->list = list;
    /* the counting pass of the grouping rides along when the indexed range is the query range (always, unless a caller narrows it) */
    if (!list) c->order_counted = c->order_ready = c->order_items = false;
    int obits = 0;
    if (!list && lo == c->q_lo && hi == c->q_hi && own_order_wanted(c, nloc, &obits) && !getenv("DISCO_NO_ORDER_FUSE")) {
        const u64 order_buckets = 1ull << obits;
        if (lo == 0 && binned_order_wanted(c, nloc, obits, &c->order_id_bits)) {
            pl->oitem = (u64 *)c->d_rec2.p;
            pl->oidbits = (u32)c->order_id_bits;
            c->order_items = true;
        } else {
            CHK(ensure(c, c->d_ocnt, order_buckets + 1));
            CHK(ensure(c, c->d_oslot, nloc));
            HIPCHK(c, hipMemsetAsync(c->d_ocnt, 0, (order_buckets + 1) * sizeof(u32), c->stream));
            pl->ocnt = c->d_ocnt;
            pl->oslot = c->d_oslot;
        }
        pl->oshift = 32u - (u32)obits;
        c->order_counted = true;
        c->order_counted_lo = lo;
        c->order_counted_hi = hi;
        c->order_counted_bits = obits;
    }
    c->runs_lpr = 0;
    c->runs_n = 0;
    c->runs_by_pos = false;
    const int nf = v.ks - v.m + 1;
    const int lpr = c->S == VERIFY_SW ? runs_lpr_for(c, nf, c->max_len, nloc) : 0;
    if (lpr && nloc) {
        CHK(ensure(c, c->d_runs, nloc * (u64)lpr));
        c->runs_lpr = lpr;
        c->runs_lo = lo;
        c->runs_n = nloc;
        c->runs_by_pos = list != nullptr;
        pl->lpr = lpr;
        pl->nf = nf;
    }
    /* the binned grouping's sub-key: index_runs_kernel knows where the read-level minimizer lies in the read, so the spare bits of the
     * item (four at 5 x 10^7 reads of 150 bases, ORDER_SUB_MAX of them taken) order the reads of a bucket by their start;
     * index_count_kernel and a full word: none */
    c->order_sub_bits = 0;
    if (pl->oitem && pl->lpr) {
        const int qbits = std::max(0, std::min(c->order_spare_bits, std::min(c->order_sub_limit, ORDER_SUB_MAX)));
        const u32 nmm_max = c->max_len - (u32)v.m + 1u; /* (lpr != 0: the longest read has a k-mer) */
        if (qbits) pl->osub = ((u32)qbits << 24) | ((1u << (qbits + 16)) / nmm_max);
        c->order_sub_bits = qbits;
    }
    return DISCO_OK;
}

/* which instantiation counts this shape — the ONLY place that names the template arguments of index_runs_kernel / index_count_kernel.
 * lpr != 0: with the minimizer runs (16 / 32 words per read: NL 1 / 2), a window of nf m-mers; long_class: the long reads of two row
 * classes, from their full rows (never with runs) */
typedef void (*IndexRunsFn)(DiscoView, u32 *, ulonglong2 *, u32 *, u64 *, u32 *, u64, u64, u32 *, u32 *, u32 *, u64 *, u32, u32, u32, const u64 *);
typedef void (*IndexCountFn)(DiscoView, u32 *, ulonglong2 *, u32 *, u64 *, u32 *, u64, u64, u32 *, u32 *, u64 *, u32, u32, const u64 *);
struct IndexCountKernel {
    IndexRunsFn runs = nullptr; /* one of the two */
    IndexCountFn plain = nullptr;
};
template <int OUT, int NF, int NFMAX, bool LONGK>
static IndexCountKernel index_runs_pick(int lpr)
{
    IndexCountKernel k;
    k.runs = lpr == 16 ? index_runs_kernel<OUT, NF, 1, NFMAX, LONGK> : index_runs_kernel<OUT, NF, 2, NFMAX, LONGK>;
    return k;
}
template <int OUT>
static IndexCountKernel index_count_pick(int nf, int m, int lpr, bool longk, bool long_class)
{
    if (long_class || !lpr) {
        IndexCountKernel k;
        if (long_class) k.plain = longk ? index_count_kernel<OUT, true, true> : index_count_kernel<OUT, false, true>;
        else k.plain = longk ? index_count_kernel<OUT, true> : index_count_kernel<OUT>;
        return k;
    }
    if (runs_nf_built(nf, m)) switch (nf) {
        case 7: return index_runs_pick<OUT, 7, 7, false>(lpr);
        case 12: return index_runs_pick<OUT, 12, 12, false>(lpr);
        case 17: return index_runs_pick<OUT, 17, 17, false>(lpr);
        case 22: return index_runs_pick<OUT, 22, 22, false>(lpr);
        default: return index_runs_pick<OUT, 27, 27, false>(lpr);
        }
    /* the window length as a run-time value: arrays for 32 or 64 m-mers */
    /* (the arrays are registers: an instantiation per size class keeps the waves per SIMD near the specialised kernels' — windows of 10
     * in arrays for 32 ran 9.8 ms at 20 M reads, in arrays for 12: 6.7) */
    if (longk) return nf <= 48 ? index_runs_pick<OUT, 0, 48, true>(lpr) : index_runs_pick<OUT, 0, 64, true>(lpr);
    if (nf <= 8) return index_runs_pick<OUT, 0, 8, false>(lpr);
    if (nf <= 12) return index_runs_pick<OUT, 0, 12, false>(lpr);
    if (nf <= 16) return index_runs_pick<OUT, 0, 16, false>(lpr);
    if (nf <= 24) return index_runs_pick<OUT, 0, 24, false>(lpr);
    if (nf <= 32) return index_runs_pick<OUT, 0, 32, false>(lpr);
    if (nf <= 48) return index_runs_pick<OUT, 0, 48, false>(lpr);
    return index_runs_pick<OUT, 0, 64, false>(lpr);
}
/* out: what the pass leaves of a read's two records (IndexOut, disco_kernels.h) — with the counting atomics on the bucket table, as plain
 * records, or as the two planes of the binned build, which counts for itself */
static IndexCountKernel index_count_pick(int out, int nf, int m, int lpr, bool longk, bool long_class)
{
    switch (out) {
    case INDEX_COUNTED: return index_count_pick<INDEX_COUNTED>(nf, m, lpr, longk, long_class);
    case INDEX_RECORDS: return index_count_pick<INDEX_RECORDS>(nf, m, lpr, longk, long_class);
    default: return index_count_pick<INDEX_PLANES>(nf, m, lpr, longk, long_class);
    }
}

/* where the count pass writes: the records of read 0 of its range as one array, or as a key plane and a payload plane */
struct IndexRecOut {
    int form = INDEX_COUNTED;
    ulonglong2 *rec = nullptr;
    u32 *key = nullptr;
    u64 *pay = nullptr;
    IndexRecOut from_read(ptrdiff_t i) const /* ... of read i */
    {
        IndexRecOut o = *this;
        if (o.rec) o.rec += 2 * i;
        if (o.key) o.key += 2 * i, o.pay += 2 * i;
        return o;
    }
};
/* a side of the partition levels' ping-pong, as the kernels' view takes it (BinxForm<R>): one array a of records, or the key plane a and
 * the payload plane b */
template <typename R>
struct BinxSide {
    typename BinxForm<R>::A *a = nullptr;
    typename BinxForm<R>::B *b = nullptr;
};
/* a side of the binned index build's ping-pong over 2n records, cut into planes: 2n payloads, then 2n keys (both 16-byte aligned) */
static BinxSide<BinxKV> index_planes(ulonglong2 *side, u64 n)
{
    BinxSide<BinxKV> s;
    s.b = (u64 *)side;
    s.a = (u32 *)(s.b + 2 * n);
    return s;
}
/* the single-GPU count pass: planes in d_rec for the binned build, counted records for the old path */
static IndexRecOut index_rec_out(disco_ctx *c)
{
    IndexRecOut o;
    if (c->binned_index) {
        const BinxSide<BinxKV> s = index_planes(c->d_rec.p, c->n);
        o.form = INDEX_PLANES;
        o.key = s.a;
        o.pay = s.b;
    } else
        o.rec = c->d_rec.p;
    return o;
}

/* reads [a, b) of the planned range; out = the records of read pl.lo */
static int index_count_chunk(disco_ctx *c, const DiscoView &v, const IndexCountPlan &pl, const IndexRecOut &out, u64 a, u64 b)
{
    if (b <= a) return DISCO_OK;
    const dim3 grid((unsigned)((b - a + 255) / 256));
    const IndexRecOut o = out.from_read((ptrdiff_t)(a - pl.lo));
    u32 *oslot = pl.oslot ? pl.oslot + (a - pl.lo) : nullptr;
    u64 *oitem = pl.oitem ? pl.oitem + (a - pl.lo) : nullptr; /* (at the read's global position, whichever chunk brings it) */
    u32 *okey = pl.list ? nullptr : c->d_okey.p; /* (a list: the keys were made when the reads were dealt, by read id) */
    const IndexCountKernel k = index_count_pick(o.form, pl.nf, v.m, pl.lpr, c->ks > 64, false);
    if (k.runs) hipLaunchKernelGGL(k.runs, grid, dim3(256), 0, c->stream, v, c->d_bkt, o.rec, o.key, o.pay, okey, a, b, c->d_runs + (a - pl.lo) * (u64)pl.lpr, pl.ocnt, oslot, oitem, pl.oidbits, pl.oshift, pl.osub, pl.list);
    else hipLaunchKernelGGL(k.plain, grid, dim3(256), 0, c->stream, v, c->d_bkt, o.rec, o.key, o.pay, okey, a, b, pl.ocnt, oslot, oitem, pl.oidbits, pl.oshift, pl.list);
    HIPCHK(c, hipGetLastError());
    return DISCO_OK;
}

/* the long reads [x_lo, x_hi) of two row classes (positions in long_ids): their records, keys and slots, from their full rows; out (the
 * records of read 0) and oslot by read id */
static int index_count_long(disco_ctx *c, const DiscoView &v, const IndexCountPlan &pl, const IndexRecOut &out, u32 *oslot, u64 x_lo, u64 x_hi)
{
    const dim3 g((unsigned)((x_hi - x_lo + 255) / 256));
    hipLaunchKernelGGL(index_count_pick(out.form, 0, v.m, 0, c->ks > 64, true).plain, g, dim3(256), 0, c->stream, v, c->d_bkt, out.rec, out.key, out.pay, c->d_okey, x_lo, x_hi, pl.ocnt, oslot,
                       (u64 *)nullptr, 0u, pl.oshift, (const u64 *)nullptr);
    HIPCHK(c, hipGetLastError());
    return DISCO_OK;
}

/* does the binned build make this index (single GPU: the only callers of index_begin)? DISCO_NO_BINNED_INDEX=1: the counting atomics,
 * the scan of the bucket table and the ordered fill, as before. The scratch side of the ping-pong is allocated here, so that a table
 * it does not fit next to takes the old path. No size policy: the index phase with the builder against the old path, same box, ms at
 * 1 / 3 / 10 / 20 / 50 M reads: 0.26 / 0.70 / 2.17 / 4.34 / 11.09 against 0.26 / 0.70 / 2.40 / 5.20 / 14.24 — no crossover, level at
 * the small sizes (profiles/binned_index_ab.txt) */
static bool binned_index_wanted(disco_ctx *c, int logT)
{
    if (getenv("DISCO_NO_BINNED_INDEX") || 2 * c->n >= 0xFFFF0000ull) return false;
    /* (2n records in planes: 2n x 12 bytes = 3n / 2 of d_rec2's 16-byte words — and never less than the n words of the grouping's items) */
    if (logT > BINX_SPAN_BITS && ensure(c, c->d_rec2, (3 * c->n + 1) / 2) != DISCO_OK) {
        (void)hipGetLastError();
        c->err.clear();
        return false;
    }
    return true;
}

/* the bucket table of an index over the context's n reads: c->T = 2^logT buckets, c->bshift; returns logT */
static int size_bucket_table(disco_ctx *c)
{
    u64 T = 1024;
    int logT = 10;
    /* records are keyed by minimizer: about one distinct key per 3-4 records at 30x. T >= 2n buckets (measured at 50 M reads:
     * n / 2n / 4n / 8n buckets -> index 15.2 / 16.4 / 18.6 / 21.0 ms, probe 47.0 / 45.6 / 45.4 / 45.4 ms) */
    double tscale = 2.0;
    if (const char *e = getenv("DISCO_BUCKET_SCALE")) tscale = atof(e);
    while ((double)T < tscale * (double)c->n && logT < 32) {
        T <<= 1;
        logT++;
    }
    c->T = T;
    c->bshift = 64 - logT;
    return logT;
}

/* sizes of the index for the context's reads and the cleared bucket table (the start of disco_build_index, or of an upload that
 * counts while it copies) */
static int index_begin(disco_ctx *c)
{
    const int logT = size_bucket_table(c);
    const u64 T = c->T;
    CHK(ensure(c, c->d_bkt, T + 1));
    CHK(ensure(c, c->d_ent, 2 * c->n));
    /* {key, record} of both end k-mers of every read, computed once by the count pass and re-read by the fill pass */
    CHK(ensure(c, c->d_rec, 2 * c->n));
    CHK(ensure(c, c->d_okey, c->n)); /* grouping keys of all reads (disco_probe orders its query range by them) */
    c->adj_imported = false;
    c->binned_index = binned_index_wanted(c, logT);
    if (!c->binned_index) HIPCHK(c, hipMemsetAsync(c->d_bkt, 0, (T + 1) * sizeof(u32), c->stream));
    return DISCO_OK;
}

/* the levels of the binned build for a table of 2^logT buckets: partitions of 2^span buckets, their prefix of logT - span bits cut into
 * `levels` digits of at most BINX_MAX_BITS bits, the first ones a bit wider where it does not divide (27: 7 + 6 over 14; 29: 8 + 7;
 * 32: 6 + 6 + 6; up to 14: no level, one partition) */
struct BinxPlan {
    int span = 0, levels = 0, bits[3] = {0, 0, 0};
};
static BinxPlan binx_plan(int logT)
{
    BinxPlan b;
    b.span = std::min(logT, BINX_SPAN_BITS);
    const int prefix = logT - b.span;
    b.levels = (prefix + BINX_MAX_BITS - 1) / BINX_MAX_BITS;
    for (int l = 0; l < b.levels; l++) b.bits[l] = prefix / b.levels + (l < prefix % b.levels ? 1 : 0);
    return b;
}

/* the partition levels over `total` records — the index's, as a key plane and a payload plane (R = BinxKV), or the grouping's
 * one-word items (u64) — whose key word holds a bucket of `bits` bits from bit kshift up (see "binned
 * index build" in disco_kernels.h): src and dst are the two sides of the ping-pong; *out = the side the partitions end up in, *part =
 * their starts (n_part + 1 words in d_binx) */
template <typename R>
static int binx_partition(disco_ctx *c, const char *what, int bits, u32 kshift, u32 total, BinxSide<R> src, BinxSide<R> dst, BinxSide<R> *out, const u32 **part)
{
    typedef typename BinxForm<R>::A A;
    typedef typename BinxForm<R>::B B;
    const BinxPlan bp = binx_plan(bits);
    const u32 n_part = 1u << (bits - bp.span);
    const u32 tiles = (total + BINX_TILE - 1u) / BINX_TILE;
    /* d_binx: seg / tb of the level at work and of the one before (n_part + 1 words each at the most), then the counts */
    u64 hist_len = 1;
    for (int l = 0, done = 0; l < bp.levels; done += bp.bits[l], l++) hist_len = std::max<u64>(hist_len, ((u64)tiles + (1ull << done)) * (1ull << bp.bits[l]) + 1);
    const u64 tab = ((u64)n_part + 1 + 63) & ~63ull;
    CHK(ensure(c, c->d_binx, 4 * tab + hist_len));
    u32 *seg[2] = {c->d_binx.p, c->d_binx.p + tab}, *tb[2] = {c->d_binx.p + 2 * tab, c->d_binx.p + 3 * tab}, *hist = c->d_binx.p + 4 * tab;
    if (getenv("DISCO_VERBOSE"))
        fprintf(stderr, "[disco] binned %s: 2^%d buckets, %u partitions of 2^%d, %d level(s) of %d / %d / %d bits\n", what, bits, n_part, bp.span, bp.levels, bp.bits[0], bp.bits[1], bp.bits[2]);
    u32 pseg = 1, pnb = 1;
    int cur = 0, done = 0;
    for (int l = 0; l < bp.levels; l++) {
        const u32 nseg = 1u << done, nb = 1u << bp.bits[l], shift = kshift + (u32)(bits - done - bp.bits[l]);
        const u32 grid = tiles + nseg;
        const u64 hlen = (u64)grid * nb + 1;
        hipLaunchKernelGGL(binx_segs_kernel, dim3(1), dim3(1024), 0, c->stream, l ? (const u32 *)hist : (const u32 *)nullptr, (const u32 *)tb[cur ^ 1], pseg, pnb, total, seg[cur], tb[cur]);
        HIPCHK(c, hipMemsetAsync(hist, 0, hlen * sizeof(u32), c->stream));
        hipLaunchKernelGGL(binx_hist_kernel<R>, dim3(grid), dim3(BINX_BLOCK), 0, c->stream, (const A *)src.a, (const u32 *)seg[cur], (const u32 *)tb[cur], nseg, shift, nb, hist);
        CHK((scan_exclusive<u32, u32>(c, hist, hlen, hist, false, nullptr)));
        hipLaunchKernelGGL(binx_scatter_kernel<R>, dim3(grid), dim3(BINX_BLOCK), 0, c->stream, (const A *)src.a, (const B *)src.b, dst.a, dst.b, (const u32 *)seg[cur], (const u32 *)tb[cur], nseg, shift, nb,
                           (const u32 *)hist);
        HIPCHK(c, hipGetLastError());
        std::swap(src, dst);
        pseg = nseg;
        pnb = nb;
        done += bp.bits[l];
        cur ^= 1;
    }
    /* the partitions' starts: the segments the last level made (no level: the one partition) */
    hipLaunchKernelGGL(binx_segs_kernel, dim3(1), dim3(1024), 0, c->stream, bp.levels ? (const u32 *)hist : (const u32 *)nullptr, (const u32 *)tb[cur ^ 1], pseg, pnb, total, seg[cur],
                       (u32 *)nullptr);
    HIPCHK(c, hipGetLastError());
    *out = src;
    *part = seg[cur];
    return DISCO_OK;
}

/* the 2n records of the count pass (INDEX_PLANES: key[i] = bucket, pay[i] = payload, in d_rec) -> bkt[0 .. T], ent[0 .. 2n); the other
 * side of the ping-pong is d_rec2, cut the same way */
static int binned_build_index(disco_ctx *c)
{
    const int logT = 64 - c->bshift;
    const u32 total = (u32)(2 * c->n);
    BinxSide<BinxKV> rec;
    const u32 *part;
    CHK(binx_partition<BinxKV>(c, "index build", logT, 0u, total, index_planes(c->d_rec.p, c->n), index_planes(c->d_rec2.p, c->n), &rec, &part));
    const int span = std::min(logT, BINX_SPAN_BITS);
    hipLaunchKernelGGL(binx_build_kernel<BinxKV>, dim3(1u << (logT - span)), dim3(BINX_BUILD_BLOCK), 0, c->stream, (const u32 *)rec.a, (const u64 *)rec.b, part, (u32)span, 0u, 0u, total, c->T,
                       c->d_bkt.p, c->d_ent.p);
    HIPCHK(c, hipGetLastError());
    return DISCO_OK;
}

/* the binned grouping: the one-word items (ORDER_ITEM) the count pass left at the start of d_rec2, one per read, -> d_order_own, the reads
 * of equal bucket back to back. The same levels and the same build kernel as the index (the order has no bucket table); the n words
 * behind the items are the other side of the ping-pong. Runs before the record build takes d_rec2. */
static int binned_build_order(disco_ctx *c)
{
    const int bits = c->order_counted_bits + c->order_sub_bits; /* (bucket and sub-key: one key) */
    const u32 total = (u32)c->n, kshift = 64u - (u32)bits;
    BinxSide<u64> items, other, rec;
    items.a = (u64 *)c->d_rec2.p;
    other.a = items.a + c->n;
    const u32 *part;
    CHK(binx_partition<u64>(c, "grouping", bits, kshift, total, items, other, &rec, &part));
    const int span = std::min(bits, BINX_SPAN_BITS);
    hipLaunchKernelGGL(binx_build_kernel<u64>, dim3(1u << (bits - span)), dim3(BINX_BUILD_BLOCK), 0, c->stream, (const u64 *)rec.a, (const u64 *)nullptr, part, (u32)span, kshift, (u32)c->order_id_bits, total, (u64)0,
                       (u32 *)nullptr, c->d_order_own.p);
    HIPCHK(c, hipGetLastError());
    return DISCO_OK;
}

/* The contained rows for the host: (id, key) of the contained reads in ascending id (scan of the flags, gather: 12 bytes per row) into
 * buffers and pinned staging memory KEPT by the context — with three allocations of up to n + 1 words, the scan and two pageable
 * copies per call this was 32 ms of the host-to-host wall at 50 M reads; now 2 ms of device work and copy + the decode. On request the
 * same rows once more in the order of the contained-read files (a counting sort by containing read on the device: the host sort took
 * 0.23 s). Started by the fetch calls, on a side stream (measured: started from disco_mark_contained, to overlap the rest of the pass, the
 * extra kernels cost the pass 0.8 ms, and 3.5 ms with the grouping — more than they hid). Single-GPU passes with up to
 * DISCO_EAGER_ROWS_MAX (16 M) contained rows; otherwise disco_fetch_contained gathers on demand the old way. */
static int start_contained_rows(disco_ctx *c, bool grouped)
{
    const u64 nc = c->n_contained;
    if (c->crows_pending && c->crows_n == nc && (!grouped || c->cgrp_pending)) return DISCO_OK; /* already on their way */
    const bool have_rows = c->crows_pending && c->crows_n == nc;
    if (!have_rows) c->crows_pending = c->cgrp_pending = false;
    const u64 max_rows = getenv("DISCO_EAGER_ROWS_MAX") ? (u64)atoll(getenv("DISCO_EAGER_ROWS_MAX")) : (16ull << 20);
    if (c->comm || nc == 0 || nc > max_rows || c->n >= (1ull << 31)) return DISCO_OK;
    if (!c->aux_stream) {
        HIPCHK(c, hipStreamCreateWithFlags(&c->aux_stream, hipStreamNonBlocking));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_crows, hipEventDisableTiming));
        HIPCHK(c, hipMalloc((void **)&c->d_total2, sizeof(u64)));
    }
    CHK(ensure(c, c->d_cpos, c->n + 1));
    CHK(ensure_group(c, nc, nc + nc / 4 + 1024, c->d_crow_id, c->d_crow_key, c->d_crow_len));
    if (nc > c->crows_hcap && c->h_ring && !c->crows_in_ring && (u64)c->ring_half * 2 >= (nc + 1024) * 32) {
        /* the pinned ring of the input stage is idle between the input stage and the text output: the rows stage there (pinning
         * 140 MB for them took 0.05 s of the host thread that feeds the pass) */
        if (c->h_crows) (void)hipHostFree(c->h_crows);
        c->h_crows = c->h_ring;
        c->crows_hcap = (u64)c->ring_half * 2 / 32;
        c->crows_in_ring = true;
    }
    if (nc > c->crows_hcap) {
        if (c->h_crows && !c->crows_in_ring) (void)hipHostFree(c->h_crows);
        c->crows_in_ring = false;
        c->h_crows = nullptr;
        c->crows_hcap = 0;
        const u64 want = nc + nc / 4 + 1024;
        if (hipHostMalloc(&c->h_crows, want * 32) != hipSuccess) { /* (both orders) no pinned memory to be had: the on-demand path */
            c->h_crows = nullptr;
            (void)hipGetLastError();
            return DISCO_OK;
        }
        c->crows_hcap = want;
    }
    if (!have_rows) {
    /* (the flags are complete: disco_mark_contained synchronised the context's stream) */
    CHK((scan_exclusive_on<u8, u32>(c, c->aux_stream, c->d_tile2, c->d_total2, c->d_contained, c->n, c->d_cpos, false, nullptr)));
    hipLaunchKernelGGL(contain_rows32_kernel, dim3(flat_grid(c, c->n)), dim3(256), 0, c->aux_stream, c->d_best, c->d_contained, c->d_cpos, c->n, c->d_crow_id, c->d_crow_key);
    HIPCHK(c, hipGetLastError());
    u64 *hkey = (u64 *)c->h_crows;
    u32 *hid = (u32 *)(hkey + c->crows_hcap), *hln = hid + c->crows_hcap;
    hipLaunchKernelGGL(crow_lens_kernel, dim3(flat_grid(c, nc)), dim3(256), 0, c->aux_stream, (const u32 *)c->d_crow_id, (const u64 *)c->d_crow_key, nc, (const u16 *)c->d_len, c->d_crow_len);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(hkey, c->d_crow_key, nc * 8, hipMemcpyDeviceToHost, c->aux_stream));
    HIPCHK(c, hipMemcpyAsync(hid, c->d_crow_id, nc * 4, hipMemcpyDeviceToHost, c->aux_stream));
    HIPCHK(c, hipMemcpyAsync(hln, c->d_crow_len, nc * 4, hipMemcpyDeviceToHost, c->aux_stream));
    HIPCHK(c, hipEventRecord(c->ev_crows, c->aux_stream));
    c->crows_n = nc;
    c->crows_pending = true;
    }
    /* ... and, on request, once more in the order of the contained-read files (crow_* kernels), behind the first copy on the same stream */
    if (grouped && !c->cgrp_pending) {
        CHK(ensure(c, c->d_cgrp_cur, c->n + 1));
        CHK(ensure_group(c, nc, nc + nc / 4 + 1024, c->d_cgrp_id, c->d_cgrp_key));
        CHK(ensure(c, c->d_cgrp_big, 1));
        HIPCHK(c, hipMemsetAsync(c->d_cpos, 0, (c->n + 1) * sizeof(u32), c->aux_stream)); /* (the flag scan has served the gather) */
        HIPCHK(c, hipMemsetAsync(c->d_cgrp_big, 0, sizeof(u64), c->aux_stream));
        hipLaunchKernelGGL(crow_count_kernel, dim3(flat_grid(c, nc)), dim3(256), 0, c->aux_stream, (const u64 *)c->d_crow_key, nc, c->d_cpos);
        CHK((scan_exclusive_on<u32, u32>(c, c->aux_stream, c->d_tile2, c->d_total2, c->d_cpos, c->n + 1, c->d_cgrp_cur, false, nullptr)));
        hipLaunchKernelGGL(crow_place_kernel, dim3(flat_grid(c, nc)), dim3(256), 0, c->aux_stream, (const u32 *)c->d_crow_id, (const u64 *)c->d_crow_key, nc, c->d_cgrp_cur, c->d_cgrp_id,
                           c->d_cgrp_key);
        hipLaunchKernelGGL(crow_sort_groups_kernel, dim3(flat_grid(c, nc)), dim3(256), 0, c->aux_stream, c->d_cgrp_id, c->d_cgrp_key, nc, c->d_cgrp_big);
        HIPCHK(c, hipGetLastError());
        u64 *gkey = (u64 *)((char *)c->h_crows + c->crows_hcap * 16);
        u32 *gid = (u32 *)(gkey + c->crows_hcap), *gln = gid + c->crows_hcap;
        /* (the lengths of the rows by id have left: their device array serves the grouped order) */
        hipLaunchKernelGGL(crow_lens_kernel, dim3(flat_grid(c, nc)), dim3(256), 0, c->aux_stream, (const u32 *)c->d_cgrp_id, (const u64 *)c->d_cgrp_key, nc, (const u16 *)c->d_len, c->d_crow_len);
        HIPCHK(c, hipMemcpyAsync(gkey, c->d_cgrp_key, nc * 8, hipMemcpyDeviceToHost, c->aux_stream));
        HIPCHK(c, hipMemcpyAsync(gid, c->d_cgrp_id, nc * 4, hipMemcpyDeviceToHost, c->aux_stream));
        HIPCHK(c, hipMemcpyAsync(gln, c->d_crow_len, nc * 4, hipMemcpyDeviceToHost, c->aux_stream));
        HIPCHK(c, hipMemcpyAsync(&c->h_cgrp_big, c->d_cgrp_big, sizeof(u64), hipMemcpyDeviceToHost, c->aux_stream));
        c->cgrp_pending = true;
    }
    return DISCO_OK;
}

/* the side stream reads best[] and the flags: nothing may rewrite them before it is done */
static int settle_contained_rows(disco_ctx *c)
{
    if (c->crows_pending) HIPCHK(c, hipStreamSynchronize(c->aux_stream));
    c->crows_pending = false;
    c->cgrp_pending = false;
    return DISCO_OK;
}

/* the pinned ring is wanted for text again (input stage, edge text): rows that stage in it and have not been fetched are given up
 * (the fetch gathers them again on demand) */
static int ring_back_from_rows(disco_ctx *c)
{
    if (!c->crows_in_ring) return DISCO_OK;
    if (c->crows_pending && c->aux_stream) HIPCHK(c, hipStreamSynchronize(c->aux_stream));
    c->crows_pending = c->cgrp_pending = false;
    c->h_crows = nullptr;
    c->crows_hcap = 0;
    c->crows_in_ring = false;
    return DISCO_OK;
}

/* the hit buffer the input stage asked for on a thread of its own: take it over (a device allocation costs 17-33 ms per GB on these
 * boxes — 0.5 to 0.9 s for the 28 GB of 50 M reads — and nothing needs the buffer before the probe) */
static void settle_hits_prealloc(disco_ctx *c)
{
    if (!c->hits_prealloc.joinable()) return;
    c->hits_prealloc.join();
    c->hbm_bytes -= std::exchange(c->prealloc_asked, 0) * 8; /* (counted when it was asked for: adopt counts what is taken over) */
    if (c->prealloc && c->prealloc.cap > c->d_hits.cap) {
        release(c, c->d_hits);
        adopt(c, c->d_hits, c->prealloc);
    } else if (c->prealloc)
        (void)hipFree(c->prealloc.p);
    c->prealloc = DevBuf<u64>();
}

/* ---- which instantiation serves a shape ---------------------------------------------------------------------------------------
 * One selector per family of templated kernels (the index count pass has its own next to index_count_chunk, above): a plain function
 * from the shape and the knobs to the kernel pointer, and the only place that names the family's template arguments. The work-queue
 * kernels are sized and launched from that one pointer (wq_launch). */

/* which instantiation probes this shape — the ONLY place that names the template arguments of probe_kernel / probe_runs_kernel.
 * mode 0: the query range (use_runs: from the minimizer runs the index pass left), 1: big_list (rows of known size), 2: slow_list */
typedef void (*ProbeFn)(ProbeArgs);
typedef void (*ProbeRunsFn)(ProbeArgs, const u32 *, u64);
struct ProbeKernel {
    ProbeRunsFn runs = nullptr; /* one of the two */
    ProbeFn plain = nullptr;
};
template <int PMODE>
static ProbeFn probe_mode_pick(bool ldsrow, bool row17, bool longk, bool long_class)
{
    if constexpr (PMODE != 0) { /* the long class does not fit the LDS row: the lists' reads from global memory */
        if (long_class) return longk ? probe_kernel<PMODE, false, false, true, true> : row17 ? probe_kernel<PMODE, false, true, false, true> : probe_kernel<PMODE, false, false, false, true>;
    }
    if constexpr (PMODE != 2) { /* (slow_list only exists next to probe_runs_kernel: 64-byte rows) */
        if (!ldsrow) return longk ? probe_kernel<PMODE, false, false, true> : row17 ? probe_kernel<PMODE, false, true> : probe_kernel<PMODE, false, false>;
    }
    return longk ? probe_kernel<PMODE, true, false, true> : row17 ? probe_kernel<PMODE, true, true> : probe_kernel<PMODE, true, false>;
}
static ProbeKernel probe_pick(const disco_ctx *c, int mode, bool use_runs)
{
    const bool ldsrow = c->S <= PROBE_ACAP; /* (two classes of rows: c->S = 8; the lists' kernels take the long class's stride into account) */
    const bool row17 = c->ks - view(c).m == 16 && !getenv("DISCO_NO_ROW17"); /* window = 17 m-mers: DPP row-scan variant */
    const bool longk = c->ks > 64;                                           /* three-word k-mers: variants of their own (kmer_is_rev) */
    const bool long_class = c->two_class && c->S_ext > PROBE_ACAP;
    ProbeKernel k;
    if (mode == 0 && use_runs) k.runs = c->k != c->ks ? (c->runs_lpr == 16 ? probe_runs_kernel<16, true> : probe_runs_kernel<32, true>) : (c->runs_lpr == 16 ? probe_runs_kernel<16> : probe_runs_kernel<32>);
    else if (mode == 0) k.plain = probe_mode_pick<0>(ldsrow, row17, longk, long_class);
    else if (mode == 1) k.plain = probe_mode_pick<1>(ldsrow, row17, longk, long_class);
    else k.plain = probe_mode_pick<2>(ldsrow, row17, longk, long_class);
    return k;
}

/* which instantiation verifies this shape, and the cap on its blocks per CU — the ONLY place that names the template arguments of
 * verify_kernel / verify_flat_kernel. mode 0: the single pass; 1 / 2: the containment-type candidates, then the overlap-type ones of
 * the non-contained reads (64-byte rows only); flat: verify_flat_kernel (64-byte rows, exact overlaps) */
typedef void (*VerifyFn)(VerifyArgs);
template <bool INEXACT>
static VerifyFn verify_rows_pick(int S, bool short_rows) /* the wave-per-read kernel by row stride */
{
    if (S == VERIFY_SW) return short_rows ? verify_kernel<5, 0, INEXACT> : verify_kernel<8, 0, INEXACT>;
    return S == 16 ? verify_kernel<16, 0, INEXACT> : S == 24 ? verify_kernel<24, 0, INEXACT> : S == 32 ? verify_kernel<32, 0, INEXACT> : verify_kernel<0, 0, INEXACT>;
}
template <int MODE>
static VerifyFn verify_pass_pick(bool flat, bool short_rows) /* a pass of the two */
{
    if (flat) return short_rows ? verify_flat_kernel<5, MODE> : verify_flat_kernel<8, MODE>;
    return short_rows ? verify_kernel<5, MODE> : verify_kernel<8, MODE>;
}
static VerifyFn verify_pick(const disco_ctx *c, int mode, bool flat, bool inexact, int *cap)
{
    const bool short_rows = c->max_len <= 160; /* rows of 5 words */
    *cap = 32;
    if (mode == 1) return verify_pass_pick<1>(flat, short_rows);
    if (mode == 2) return verify_pass_pick<2>(flat, short_rows);
    if (inexact) return verify_rows_pick<true>(c->S, short_rows);
    if (!flat) return verify_rows_pick<false>(c->S, short_rows);
    /* pairs of batches share their row fetches (verify_flat_kernel<·, 0, true>): 21.5 against 22.6 ms and 18 GB less traffic at config 3
     * (reads of up to 160 bases); 32.3 against 33.0–35.1 ms on 50 M reads of 100–250 bases, 72.9 against 76.3 with config 5's
     * abundances (256-base rows, 15 KB of LDS per wavefront). DISCO_VERIFY_CACHE=0 forbids it */
    const char *vce = getenv("DISCO_VERIFY_CACHE");
    const bool vcache = vce ? atoi(vce) != 0 : true;
    if (!vcache) return short_rows ? verify_flat_kernel<5> : verify_flat_kernel<8>;
    /* (round 5: 128 registers and 10 KB of LDS hold sixteen blocks per CU; 12 / 14 / 16 resident: 22.8 / 21.5 / 22.0 ms — the rows of
     * sixteen blocks' pairs no longer shared the L2 as well. Round 6: with the work queue split by XCD (wq_grab_split: an XCD's waves
     * work through one contiguous eighth of the processing order) 12 / 14 / 16: 22.7 / 20.8 / 19.8 ms — all sixteen) */
    if (short_rows) *cap = 16;
    return short_rows ? verify_flat_kernel<5, 0, true> : verify_flat_kernel<8, 0, true>;
}
static void verify_launch(disco_ctx *c, const VerifyArgs &va, u64 nq, int mode, bool flat, bool inexact)
{
    int cap = 0;
    const VerifyFn k = verify_pick(c, mode, flat, inexact, &cap);
    wq_launch(c, k, nq, "DISCO_VERIFY_WAVES", cap, va);
}

/* which instantiation selects the edges — the ONLY place that names the template arguments of edge_select_flat_kernel /
 * edge_select_kernel. big: the rows of the big-row list, one per grab; flat: the hits of several reads as one flat list; small: its
 * variant with five waves per SIMD */
typedef void (*EdgeSelFn)(EdgeSelArgs);
/* sub-chunks of up to 4 rows / 4 batches: 9.7 KB of LDS, 16 waves per CU. Larger ones fill their last batch better and repeat the
 * per-sub-chunk work less often (8 rows: 140 instead of 175 vector instructions per read) but hold 11 waves per CU, and the kernel's
 * time follows the resident waves (LDS round trips between its phases): 8 x 4: 25.4 ms, 4 x 4: 19.2 ms at 50 M reads */
/* (round 6: sub-chunks of 4 rows x 3 batches — 16.35 against 17.1 ms with 3 x 2; in round 5 that shape spilled three registers with the
 * sequential path compiled in, the branch-free load pipeline made room; 4 x 4, 5 x 3 and 5 x 4 still spill 12 / 3 / 17) */
#ifndef SEL_SMALL_ROWS
#define SEL_SMALL_ROWS 4
#define SEL_SMALL_NB 3
#endif
static EdgeSelFn edge_select_pick(bool big, bool flat, bool small)
{
    if (big) return edge_select_kernel<true>;
    if (flat) return small ? edge_select_flat_kernel<SEL_SMALL_ROWS, SEL_SMALL_NB, true> : edge_select_flat_kernel<4, 4>;
    return edge_select_kernel<false>;
}

/* which instantiation marks the transitive edges — the ONLY place that names the template arguments of transitive_mark_kernel.
 * big: the nodes of the big-node list (hash tables in global scratch); defer: the multi-rank kernel (a node short of a row waits for the
 * request-all round; its first pass always with the small arrays); small: LDS arrays for TR_CAP_SMALL neighbours (eight waves per
 * SIMD); lists: the survivor lists are the result */
typedef void (*TrFn)(TrArgs);
static TrFn tr_pick(bool big, bool defer, bool small, bool lists)
{
    if (big) return defer ? transitive_mark_kernel<true, true> : transitive_mark_kernel<true, false>;
    if (defer) return lists ? transitive_mark_kernel<false, true, TR_CAP_SMALL, true> : transitive_mark_kernel<false, true, TR_CAP_SMALL>;
#if defined(TR_EXP_DEFER_SINGLE) /* timing experiment: the multi-rank variant of the kernel on one GPU's nodes */
    if (small) return transitive_mark_kernel<false, true, TR_CAP_SMALL>;
#else
    if (small) return lists ? transitive_mark_kernel<false, false, TR_CAP_SMALL, true> : transitive_mark_kernel<false, false, TR_CAP_SMALL>;
#endif
    return transitive_mark_kernel<false, false>;
}

/* the fields of TrArgs both marking drivers fill alike, after the big-node list has its size; c->use_half: the survivor lists and the
 * list of wide nodes, cleared (order and all_flags are the caller's); selfdel: the lists carry their own end, no count is kept */
static int tr_args_begin(disco_ctx *c, TrArgs *a, bool selfdel = false)
{
    a->v = view(c);
    a->ref = c->d_adj_ref;
    a->adj = c->d_adj;
    a->big_list = c->d_big_list;
    a->n_big = c->d_n_big;
    a->big_cap = c->d_big_list.cap;
    a->scratch = nullptr;
    a->hcap = 0;
    a->half = nullptr;
    a->hcnt = nullptr;
    if (c->use_half) {
        CHK(ensure(c, c->d_half, c->n * HALF_CAP));
        if (!selfdel) { /* (self-delimiting lists: no count — neither the 4 bytes per node nor their clearing every pass) */
            CHK(ensure(c, c->d_hcnt, c->n));
            HIPCHK(c, hipMemsetAsync(c->d_hcnt, 0, std::max<u64>(c->n, 1) * sizeof(u32), c->stream));
        }
        CHK(ensure(c, c->d_wide, std::min<u64>(c->n, c->n / 32 + 4096)));
        CHK(ensure(c, c->d_n_wide, 1));
        HIPCHK(c, hipMemsetAsync(c->d_n_wide, 0, sizeof(u32), c->stream));
        a->half = c->d_half;
        a->hcnt = selfdel ? nullptr : (u32 *)c->d_hcnt;
    }
    c->half_selfdel = c->use_half && selfdel;
    a->wide_list = c->d_wide;
    a->n_wide = c->d_n_wide;
    a->wide_cap = c->d_wide.cap;
    return DISCO_OK;
}

/* the big-node pass of the marking: the n_big nodes of big_list through hash tables in global scratch. It may raise CTR_OVERFLOW (read
 * back here: the caller says what that means) */
static int tr_big_nodes(disco_ctx *c, TrArgs *a, u32 n_big, bool defer, const char *what)
{
    /* longest list among the big nodes bounds the hash size: one reduction on the device, one read-back */
    CHK(zero_counter(c, CTR_MAX_DEG));
    hipLaunchKernelGGL(list_max_degree_kernel, dim3(flat_grid(c, n_big)), dim3(256), 0, c->stream, c->d_big_list, (u64)n_big, c->d_adj_ref, c->d_ctr + CTR_MAX_DEG);
    HIPCHK(c, hipGetLastError());
    CHK(read_counters(c));
    const u64 maxd = c->h_ctr[CTR_MAX_DEG];
    u64 hcap = 64;
    while (hcap < 2 * maxd) hcap <<= 1;
    const int g2 = (int)std::min<u64>(n_big, (u64)c->n_cu * 8);
    const u64 per = hcap * 8 + hcap * 4 + hcap;
    LocalBuf<u8> scratch(c);
    CHK(ensure(c, scratch, (u64)g2 * per));
    a->scratch = (u64 *)scratch.p;
    a->hcap = hcap;
    a->adj = c->d_adj; /* (multi-rank: the array may have moved — adj_tail_reserve) */
    HIPCHK(c, hipMemsetAsync(c->d_wq, 0, sizeof(u64) * WQ_WORDS, c->stream));
    hipLaunchKernelGGL(tr_pick(true, defer, false, false), dim3(g2), dim3(64), 0, c->stream, *a);
    const hipError_t e = hipGetLastError();
    const int rc = read_counters(c); /* synchronises before the scratch goes back */
    if (e != hipSuccess) return fail(c, DISCO_E_HIP, "transitive_mark_kernel (%s): %s", what, hipGetErrorString(e));
    return rc;
}

static int dist_mark_contained(disco_ctx *c); /* multi-GPU flow, below */
static int dist_partitioned_probe(disco_ctx *c);

/* ================================================================================================================ */
extern "C" {

int disco_abi_version(void) { return DISCO_ABI_VERSION; }

int disco_create(int device, const disco_params *p, disco_ctx **out)
{
    if (!p || !out) return fail(nullptr, DISCO_E_ARG, "disco_create: null argument");
    /* (a longer k-mer: only for a caller who asks for the seeded index — every length a read can have is then accepted, and the reads'
     * own validation, min_overlap < length <= 32767, is the bound) */
    if (p->min_overlap < 2 || (p->min_overlap - 1 > DISCO_MAX_K && !(p->flags & DISCO_FLAG_SEEDED_KMER)))
        return fail(nullptr, DISCO_E_UNSUPPORTED, "disco_create: min_overlap %u unsupported (k = min_overlap-1 must be in [1,%d])", p->min_overlap, DISCO_MAX_K);
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) return fail(nullptr, DISCO_E_HIP, "disco_create: no HIP device (%s)", hipGetErrorString(e));
    if (device < 0 || device >= ndev) return fail(nullptr, DISCO_E_ARG, "disco_create: device %d out of range (%d devices)", device, ndev);
    disco_ctx *c = new (std::nothrow) disco_ctx();
    if (!c) return fail(nullptr, DISCO_E_NOMEM, "disco_create: out of host memory");
    c->device = device;
    c->prm = *p;
    if (c->prm.max_edges_per_kmer == 0) c->prm.max_edges_per_kmer = 4;
    if (c->prm.max_substitutions > 32767) c->prm.max_substitutions = 32767; /* no read is longer (15-bit length field) */
    c->k = (int)p->min_overlap - 1;
    c->ks = std::min(c->k, DISCO_MAX_K);
#define CREATE_CHK(call)                                                                              \
    do {                                                                                              \
        hipError_t e2 = (call);                                                                       \
        if (e2 != hipSuccess) {                                                                       \
            int rc = fail(nullptr, DISCO_E_HIP, "disco_create: %s failed: %s", #call, hipGetErrorString(e2)); \
            delete c;                                                                                 \
            return rc;                                                                                \
        }                                                                                             \
    } while (0)
    CREATE_CHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    CREATE_CHK(hipGetDeviceProperties(&prop, device));
    c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    CREATE_CHK(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
    CREATE_CHK(hipMalloc((void **)&c->d_ctr, sizeof(u64) * CTR_COUNT));
    CREATE_CHK(hipMemset(c->d_ctr, 0, sizeof(u64) * CTR_COUNT));
    CREATE_CHK(hipMalloc((void **)&c->d_total, sizeof(u64)));
    CREATE_CHK(hipMalloc((void **)&c->d_wq, sizeof(u64) * WQ_WORDS)); /* (WQ_NQ sub-queues, a 128-byte slot each: wq_grab_split) */
    CREATE_CHK(hipMalloc((void **)&c->d_bump, sizeof(u64)));
    CREATE_CHK(hipMalloc((void **)&c->d_n_big, sizeof(u32)));
    CREATE_CHK(hipMalloc((void **)&c->d_n_slow, sizeof(u32)));
    CREATE_CHK(hipMalloc((void **)&c->d_n_extra, sizeof(u32)));
    for (int i = 0; i < DISCO_PH_SLOTS; i++) {
        CREATE_CHK(hipEventCreate(&c->ev0[i]));
        CREATE_CHK(hipEventCreate(&c->ev1[i]));
    }
#undef CREATE_CHK
    *out = c;
    return DISCO_OK;
}

void disco_destroy(disco_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    free_graph_state(c);
    free_reads(c);
    release(c, c->d_tile);
    (void)hipFree(c->d_ctr);
    (void)hipFree(c->d_total);
    (void)hipFree(c->d_wq);
    (void)hipFree(c->d_bump);
    if (c->h_stage) (void)hipHostFree(c->h_stage);
    for (int i = 0; i < 2; i++)
        if (c->ev_stage[i]) (void)hipEventDestroy(c->ev_stage[i]);
    (void)hipFree(c->d_n_big);
    (void)hipFree(c->d_n_slow);
    (void)hipFree(c->d_n_extra);
    release(c, c->d_probe_rare);
    release(c, c->d_route);
    release(c, c->d_list_n);
    delete c->comm_bulk;
    delete c->comm;
    c->comm = c->comm_bulk = nullptr;
    if (c->bulk_stream) (void)hipStreamDestroy(c->bulk_stream);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->aux_stream) {
        (void)hipStreamSynchronize(c->aux_stream);
        (void)hipStreamDestroy(c->aux_stream);
        (void)hipEventDestroy(c->ev_crows);
        (void)hipFree(c->d_total2);
    }
    release(c, c->d_tile2);
    release(c, c->d_cpos);
    release(c, c->d_crow_id);
    release(c, c->d_crow_key);
    release(c, c->d_crow_len);
    release(c, c->d_cgrp_cur);
    release(c, c->d_cgrp_id);
    release(c, c->d_cgrp_key);
    release(c, c->d_cgrp_big);
    release(c, c->d_fetch_src);
    release(c, c->d_fetch_ent);
    if (c->h_crows && !c->crows_in_ring) (void)hipHostFree(c->h_crows);
    settle_hits_prealloc(c);
    release(c, c->d_ingest);
    if (c->h_ring) (void)hipHostFree(c->h_ring);
    for (int i = 0; i < 2; i++)
        if (c->ev_ring[i]) (void)hipEventDestroy(c->ev_ring[i]);
    release(c, c->d_rec_of_read);
    for (int i = 0; i < 3; i++) {
        if (c->ev_copied[i]) (void)hipEventDestroy(c->ev_copied[i]);
        if (c->ev_unpacked[i]) (void)hipEventDestroy(c->ev_unpacked[i]);
    }
    if (c->ev_bulk) (void)hipEventDestroy(c->ev_bulk);
    if (c->ev_keys) (void)hipEventDestroy(c->ev_keys);
    if (c->ev_keys_go) (void)hipEventDestroy(c->ev_keys_go);
    for (int i = 0; i < DISCO_PH_SLOTS; i++) {
        if (c->ev0[i]) (void)hipEventDestroy(c->ev0[i]);
        if (c->ev1[i]) (void)hipEventDestroy(c->ev1[i]);
    }
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    if (c->arena.base) (void)hipFree(c->arena.base); /* (every buffer carved out of it was released above or dies with it) */
    delete c;
}

const char *disco_last_error(const disco_ctx *c) { return c ? c->err.c_str() : g_create_error.c_str(); }

int disco_set_stream(disco_ctx *c, void *hip_stream)
{
    if (!c) return DISCO_E_ARG;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    return DISCO_OK;
}

int disco_synchronize(disco_ctx *c)
{
    if (!c) return DISCO_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DISCO_OK;
}

int disco_pack_ascii(const char *seq, uint32_t len, uint64_t *out_words)
{
    if (!seq || !out_words) return DISCO_E_ARG;
    uint32_t nw = (len + 31) / 32;
    for (uint32_t w = 0; w < nw; w++) out_words[w] = 0;
    for (uint32_t i = 0; i < len; i++) {
        uint64_t b;
        switch (seq[i]) {
        case 'A': b = 0; break;
        case 'C': b = 1; break;
        case 'G': b = 2; break;
        case 'T': b = 3; break;
        default: return DISCO_E_ARG;
        }
        out_words[i >> 5] |= b << (62 - 2 * (i & 31));
    }
    return DISCO_OK;
}

void *disco_host_alloc(size_t bytes)
{
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}

void disco_host_free(void *p)
{
    if (p) (void)hipHostFree(p);
}

/* keep != null: the caller owns-and-fills the table itself (upload, generator). If the context already holds an owned table of exactly
 * this shape, NOTHING is freed — table, index, hit buffer, lists all keep their size and the next pass finds them as a repeated pass
 * does (*keep = true); dropping and re-allocating tens of GB per read set cost 60 ms at best and, on some boxes, 1.2–1.9 s in the
 * first allocation afterwards */
static int set_reads_common(disco_ctx *c, u64 n, uint32_t stride, bool *keep = nullptr)
{
    if (n >= (1ull << 31)) return fail(c, DISCO_E_UNSUPPORTED, "more than 2^31 reads per context are not supported");
    if (stride == 0 || stride > 1024) return fail(c, DISCO_E_ARG, "stride_words %u out of range", stride);
    c->index_counted = false;
    if (c->crows_pending && c->aux_stream) (void)hipStreamSynchronize(c->aux_stream);
    c->crows_pending = false;
    c->cgrp_pending = false;
    const bool kept = keep && c->reads_owned && !c->two_class && !c->dist_reads && !c->comm && c->d_reads && c->d_len && n > 0 && c->n == n && c->n_alloc == n &&
                      c->S == (int)stride && !getenv("DISCO_NO_BUFFER_REUSE");
    if (keep) *keep = kept;
    if (kept) {
        c->h_len_ok = false; /* (not cleared: the next upload overwrites it in place) */
        c->n_out = c->out_used = 0;
        c->adj_total = 0;
        c->flags_pending = false;
        c->adj_imported = false;
        c->ch_ready = false;
        c->d_adj = nullptr;
        c->d_order_used = nullptr;
    } else {
        free_graph_state(c);
        free_reads(c);
        c->n = n;
        c->n_alloc = n;
        c->dist_reads = false;
        c->S = (int)stride;
    }
    c->dist_active = false;
    c->q_lo = 0;
    c->q_hi = n;
    c->phase = 0;
    return DISCO_OK;
}

/* the copy stream and its events (first use) */
static int ensure_copy_stream(disco_ctx *c)
{
    if (c->copy_stream) return DISCO_OK;
    HIPCHK(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    for (int i = 0; i < 3; i++) {
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_copied[i], hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_unpacked[i], hipEventDisableTiming));
    }
    return DISCO_OK;
}

/* the copy stream starts behind whatever the context's stream still holds (a pass the caller did not wait for may be reading the
 * table, or the memory the copies are about to fill) */
static int copy_stream_after_stream(disco_ctx *c)
{
    HIPCHK(c, hipEventRecord(c->ev_unpacked[0], c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->copy_stream, c->ev_unpacked[0], 0));
    return DISCO_OK;
}

/* the device's check of the lengths of the reads [lo, hi): h_ctr[CTR_BAD_LEN / CTR_MAX_LEN / CTR_MIN_LEN (complemented)] on return */
static int count_lengths(disco_ctx *c, u64 lo, u64 hi)
{
    CHK(zero_counter(c, CTR_BAD_LEN));
    CHK(zero_counter(c, CTR_MAX_LEN));
    CHK(zero_counter(c, CTR_MIN_LEN));
    if (hi > lo) hipLaunchKernelGGL(validate_len_kernel, dim3(flat_grid(c, hi - lo)), dim3(256), 0, c->stream, c->d_len + lo, hi - lo, c->S, (int)c->prm.min_overlap, c->d_ctr);
    return read_counters(c);
}

static int validate_reads(disco_ctx *c)
{
    CHK(count_lengths(c, 0, c->n));
    c->min_len = 0xFFFFu - (u32)c->h_ctr[CTR_MIN_LEN];
    if (c->h_ctr[CTR_BAD_LEN])
        return fail(c, DISCO_E_ARG, "%llu reads have a length outside (min_overlap=%u, min(32767, 32*stride)]", (unsigned long long)c->h_ctr[CTR_BAD_LEN], c->prm.min_overlap);
    c->max_len = (u32)c->h_ctr[CTR_MAX_LEN];
    c->phase = 1;
    return DISCO_OK;
}

/* ---- where a read table begins -------------------------------------------------------------------------------------------------
 * Every producer of a table comes here for the layout, the release of the old table, ownership, the buffers and the meaning of the
 * length fields; what it then does is fill. ReadShape: what a producer knows of its reads before it touches the context (a generator
 * knows n and the stride: validate_reads has the rest) */
struct ReadShape {
    u64 n = 0;
    uint32_t stride = 0; /* words of a row that holds the longest read, padded to 64 bytes */
    u64 n_long = 0;      /* reads of more than DISCO_SHORT_MAX bases */
    u32 short_max = 0, longest = 0, shortest = 0; /* short_max: the longest of the others */
};

/* the length fields: under two classes of rows max_len is the SHORT class's longest read (its paths are those of a pure short set) */
static void set_read_lengths(disco_ctx *c, u32 longest, u32 short_max, u32 shortest)
{
    c->max_len_all = longest;
    c->max_len = c->two_class ? short_max : longest;
    c->min_len = shortest;
}

/* a refused read set leaves the context with no reads: the stride of the empty table is any valid one (a bad length may ask for more
 * than set_reads_common accepts, and its refusal would leave the PREVIOUS reads and graph in place) */
static void drop_reads(disco_ctx *c) { (void)set_reads_common(c, 0, VERIFY_SW, nullptr); }

/* the one-stride part: the old table goes (may_keep: or stays, if it is the context's own of this shape), and n_alloc rows of `stride`
 * words (extra_rows more: the long class's tail rows) with n_alloc lengths are the context's own — flagged so only once the old table is
 * released: an adopted one is never freed, kept or written. spare_hits: the hit buffer is in use (the input stage's arena may be it) and
 * survives the release of the graph state of a read set of another shape */
static int begin_rows(disco_ctx *c, u64 n, u64 n_alloc, u64 extra_rows, uint32_t stride, bool may_keep, bool spare_hits = false)
{
    LocalBuf<u64> hits(c);
    bool kept = false;
    if (spare_hits) hits.take(c->d_hits);
    const int rc = set_reads_common(c, n, stride, may_keep ? &kept : nullptr);
    if (spare_hits) hits.give(c->d_hits);
    CHK(rc);
    c->reads_owned = true; /* whatever is allocated from here on is released by free_reads */
    c->n_alloc = n_alloc;
    return kept ? DISCO_OK : alloc_reads(c, (n_alloc + extra_rows) * (u64)stride, n_alloc);
}

/* a table of the context's own for reads of this shape, up to "the buffers exist"; an own table of the same shape is kept. A few long reads
 * among short ones: two classes of rows (c->two_class on return) — the table of one stride, n rows as wide as the longest read, is never made */
static int begin_read_table(disco_ctx *c, const ReadShape &s, bool spare_hits = false)
{
    const bool classes = two_class_ok(c, (int)s.stride, s.n, s.n_long, s.short_max, true);
    CHK(begin_rows(c, s.n, s.n, classes ? s.n_long : 0, classes ? (uint32_t)VERIFY_SW : s.stride, !classes, spare_hits));
    if (classes) CHK(two_class_alloc(c, s.n_long, (int)s.stride, s.short_max));
    set_read_lengths(c, s.longest, s.short_max, s.shortest);
    return DISCO_OK;
}

/* the long reads' numbers: ovf[i] = long reads before read i (the flags, scanned in place; CTR_SHORT_MAX takes the longest of the others)
 * and, where asked, ids[x] = the read that is long read x. count == null: nothing waits for the device (an upload issues its chunks behind this) */
static int number_long_reads(disco_ctx *c, u32 *ovf, u32 *ids, u64 *count)
{
    hipLaunchKernelGGL(class_flag_kernel, dim3(flat_grid(c, c->n)), dim3(256), 0, c->stream, (const u16 *)c->d_len, c->n, ovf, c->d_ctr);
    CHK((scan_exclusive<u32, u32>(c, ovf, c->n, ovf, false, count)));
    if (ids) hipLaunchKernelGGL(class_ids_kernel, dim3(flat_grid(c, c->n)), dim3(256), 0, c->stream, (const u16 *)c->d_len, (const u32 *)ovf, c->n, ids);
    return DISCO_OK;
}

/* disco_upload_reads (stride_words > 0: one stride on the host) and disco_upload_reads_ragged (stride_words = 0: the reads back to back,
 * ceil(len / 32) words each — the form the reference itself keeps them in, BG/HashTable.cpp:456-477) */
static int upload_reads_impl(disco_ctx *c, const char *who, const uint64_t *packed, uint32_t stride_words, const uint16_t *len, uint64_t n)
{
    if (!c || (n && (!packed || !len))) return c ? fail(c, DISCO_E_ARG, "%s: null argument", who) : DISCO_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const bool ragged = stride_words == 0;
    const auto t_begin = std::chrono::steady_clock::now();
    auto lapms = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count(); };
    double t_scan = 0, t_alloc = 0, t_issued = 0, t_mirror = 0;
    u64 CH = getenv("DISCO_UPLOAD_CHUNK") ? (u64)atoll(getenv("DISCO_UPLOAD_CHUNK")) : (4ull << 20);
    if (!ragged) CH = std::min<u64>(CH, (512ull << 20) / ((u64)stride_words * 8)); /* (a chunk of wide rows: at most 512 MB per staging buffer) */
    CH = std::max<u64>((CH + 255) & ~255ull, 256);
    const u64 n_chunks = (n + CH - 1) / CH;
    /* the lengths are checked where they are (the host has them): min_overlap < len <= min(32767, 32 * stride) (BG/Dataset.cpp:305,
     * BG/HashTable.cpp:531); longest / shortest decide the kernel variants of the pass, the long reads the layout; ragged: the words of
     * every chunk of CH reads */
    u64 n_bad = 0;
    ReadShape shape{n, 0, 0, 0, 0, n ? 0xFFFFu : 0u};
    std::vector<u64> chunk_words(n_chunks + 1, 0);
    {
        const u32 mo = c->prm.min_overlap, cap = ragged ? 32767u : std::min<u32>(32767u, stride_words * 32u);
        std::mutex mu;
        parallel_for(n, [&](u64 b0, u64 e0) {
            u64 bad = 0, nlong = 0;
            u32 mx = 0, mn = 0xFFFFu, smx = 0;
            for (u64 k = b0 / CH; k * CH < e0; k++) { /* the piece of chunk k inside [b0, e0) */
                u64 words = 0;
                for (u64 i = std::max<u64>(b0, k * CH); i < std::min<u64>(e0, (k + 1) * CH); i++) {
                    const u32 L = len[i];
                    bad += (L <= mo || L > cap);
                    mx = std::max(mx, L);
                    mn = std::min(mn, L);
                    nlong += L > (u32)DISCO_SHORT_MAX;
                    if (L <= (u32)DISCO_SHORT_MAX) smx = std::max(smx, L);
                    words += (L + 31u) >> 5;
                }
                std::lock_guard<std::mutex> lk(mu);
                chunk_words[k + 1] += words;
            }
            std::lock_guard<std::mutex> lk(mu);
            n_bad += bad;
            shape.n_long += nlong;
            shape.longest = std::max(shape.longest, mx);
            shape.shortest = std::min(shape.shortest, mn);
            shape.short_max = std::max(shape.short_max, smx);
        });
        for (u64 k = 0; k < n_chunks; k++) chunk_words[k + 1] += chunk_words[k];
    }
    if (ragged) stride_words = std::max<u32>(1, (shape.longest + 31) / 32);
    t_scan = lapms();
    /* rows are padded to a multiple of 8 words = 64 B so that a candidate row fetch touches whole, aligned HBM sectors */
    const uint32_t dstride = shape.stride = (stride_words + 7u) & ~7u;
    if (n_bad) {
        drop_reads(c);
        return fail(c, DISCO_E_ARG, "%llu reads have a length outside (min_overlap=%u, min(32767, 32*stride)]", (unsigned long long)n_bad, c->prm.min_overlap);
    }
    CHK(begin_read_table(c, shape));
    const bool classes = c->two_class; /* (the chunks are then unpacked per class) */
    if (n) {
        /* The copy runs in chunks on a stream of its own; behind it, chunk by chunk on the context's stream: rows spread to the 64-byte
         * stride of the table (host rows at the words they use: 5 of 8 at 150 bp — 2.0 instead of 3.2 GB over the link; a 2-D copy of 40-byte
         * rows ran at 8.7 GB/s) and the COUNT PASS OF THE INDEX over the chunk's reads (index_runs_kernel: 9 ms at 50 M reads, hidden behind
         * the 38 ms of the copy) — disco_build_index then starts at its scan. The call returns when the host buffer is free again. */
        CHK(ensure_copy_stream(c));
        CHK(copy_stream_after_stream(c));
        const bool direct = !ragged && !classes && dstride == stride_words; /* the host rows ARE the table's rows: copied where they belong */
        /* (two classes: the index is counted by disco_build_index, over the classes) */
        const bool eager = !c->comm && !classes && !getenv("DISCO_NO_EAGER_INDEX");
        HIPCHK(c, hipMemcpyAsync(c->d_len, len, n * 2, hipMemcpyHostToDevice, c->stream));
        u64 ring_words = 0; /* words of the largest chunk as it lies on the host */
        for (u64 k = 0; k < n_chunks; k++)
            ring_words = std::max<u64>(ring_words, ragged ? chunk_words[k + 1] - chunk_words[k] : (std::min<u64>(n, (k + 1) * CH) - k * CH) * (u64)stride_words);
        if (!direct) CHK(ensure(c, c->d_dense, 3 * ring_words));
        LocalBuf<u64> woff(c);
        LocalBuf<u32> nw(c);
        if (ragged) { /* word offset of every read: scan of ceil(len / 32) */
            CHK(ensure(c, woff, n));
            CHK(ensure(c, nw, n));
            hipLaunchKernelGGL(words_per_read_kernel, dim3(flat_grid(c, n)), dim3(256), 0, c->stream, (const u16 *)c->d_len, n, nw);
            CHK((scan_exclusive<u32, u64>(c, nw, n, woff, false, nullptr)));
        }
        if (classes) CHK(number_long_reads(c, c->d_ovf, c->d_long_ids, nullptr));
        t_alloc = lapms();
        IndexCountPlan pl;
        DiscoView v;
        if (eager) {
            CHK(index_begin(c));
            v = view(c);
            CHK(index_count_plan(c, v, 0, n, &pl));
        }
        for (u64 k = 0; k < n_chunks; k++) {
            const u64 lo = k * CH, hi = std::min<u64>(n, lo + CH);
            const int b = (int)(k % 3);
            if (!direct) {
                u64 *ring = c->d_dense + (u64)b * ring_words;
                const u64 w0 = ragged ? chunk_words[k] : lo * (u64)stride_words, w1 = ragged ? chunk_words[k + 1] : hi * (u64)stride_words;
                if (k >= 3) HIPCHK(c, hipStreamWaitEvent(c->copy_stream, c->ev_unpacked[b], 0));
                HIPCHK(c, hipMemcpyAsync(ring, packed + w0, (w1 - w0) * 8, hipMemcpyHostToDevice, c->copy_stream));
                HIPCHK(c, hipEventRecord(c->ev_copied[b], c->copy_stream));
                HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_copied[b], 0));
                hipLaunchKernelGGL(unpack_reads_kernel, dim3(flat_grid(c, (hi - lo) * (u64)c->S)), dim3(256), 0, c->stream, (const u64 *)ring, ragged ? 0 : (int)stride_words, (const u64 *)woff, w0,
                                   (const u16 *)c->d_len, lo, hi, c->S, classes ? (u32)DISCO_SHORT_MAX : 0xFFFFu, c->d_reads);
                if (classes)
                    hipLaunchKernelGGL(unpack_long_reads_kernel, dim3(flat_grid(c, shape.n_long * ((u64)dstride + 8))), dim3(256), 0, c->stream, (const u64 *)ring, ragged ? 0 : (int)stride_words,
                                       (const u64 *)woff, w0, (const u16 *)c->d_len, lo, hi, (const u32 *)c->d_long_ids, shape.n_long, n, (int)dstride, c->tailb, c->d_full, c->d_reads);
                HIPCHK(c, hipEventRecord(c->ev_unpacked[b], c->stream));
            } else { /* (one 1-D copy per chunk: a 2-D copy whose width equals both pitches ran at a third of the rate) */
                HIPCHK(c, hipMemcpyAsync(c->d_reads + lo * dstride, packed + lo * dstride, (hi - lo) * (u64)dstride * 8, hipMemcpyHostToDevice, c->copy_stream));
                HIPCHK(c, hipEventRecord(c->ev_copied[b], c->copy_stream));
                HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_copied[b], 0));
            }
            if (eager) CHK(index_count_chunk(c, v, pl, index_rec_out(c), lo, hi));
        }
        HIPCHK(c, hipGetLastError());
        t_issued = lapms();
        /* the host's copy of the lengths (result decoding) while the chunks travel */
        if (c->h_len.size() != n) c->h_len.resize(n);
        uint16_t *hl = c->h_len.data();
        parallel_for(n, [&, hl](u64 b0, u64 e0) { memcpy(hl + b0, len + b0, (e0 - b0) * 2); });
        c->h_len_ok = true;
        t_mirror = lapms();
        HIPCHK(c, hipStreamSynchronize(c->copy_stream));
        if (getenv("DISCO_VERBOSE"))
            fprintf(stderr, "[disco] %s: lengths checked %.1f ms, buffers %.1f, chunks issued %.1f, lengths mirrored %.1f, copies done %.1f (%s%s)\n", who, t_scan, t_alloc, t_issued,
                    t_mirror, lapms(), classes ? "two classes of rows" : "one stride", eager ? ", index counted behind the copies" : "");
        if (woff) HIPCHK(c, hipStreamSynchronize(c->stream)); /* (read by the unpack kernels on the context's stream; it goes with this block) */
        c->index_counted = eager;
    } else
        c->h_len.clear();
    c->phase = 1;
    return DISCO_OK;
}

int disco_upload_reads(disco_ctx *c, const uint64_t *packed, uint32_t stride_words, const uint16_t *len, uint64_t n)
{
    DISCO_TRACE("disco_upload_reads");
    if (c && stride_words == 0) return fail(c, DISCO_E_ARG, "stride_words 0 out of range");
    return upload_reads_impl(c, "disco_upload_reads", packed, stride_words, len, n);
}

int disco_upload_reads_ragged(disco_ctx *c, const uint64_t *words, const uint16_t *len, uint64_t n)
{
    DISCO_TRACE("disco_upload_reads_ragged");
    return upload_reads_impl(c, "disco_upload_reads_ragged", words, 0, len, n);
}

/* ================================================================================================================
 * input stage on the GPU (kernels: disco_ingest.h)
 * ============================================================================================================== */
namespace {
/* figures of a piece's records: what its filter leaves and, under a communicator, what the ranks exchange */
enum { DP_STARTS = 0, DP_GOOD, DP_TOO_LONG, DP_MAX_LEN, DP_MIN_LEN_INV, DP_N_LONG, DP_SHORT_MAX, DP_COUNT };

/* the part of a file one job works on (kernels: disco_ingest.h). One GPU: the whole file; under a communicator: the rank's share of its bytes */
struct IngestPiece {
    u64 p0 = 0, p1 = 0;                /* the owned bytes of the file */
    u64 own_lo = 0, own_hi = 0, n = 0; /* the same in the buffer, and the buffer's bytes */
    bool to_eof = false;               /* the buffer reaches the end of the file */
    bool prefix_nl = true, last_nl = false; /* the byte in front of the piece (the file's first byte: nothing counts as one) / its last byte is a newline */
    u64 own_nl = 0, tiles = 0;
    u8 *d_text = nullptr;
    u64 *d_tile_base = nullptr, *d_ctr = nullptr; /* d_ctr: the kernels' counters (FX_CTR_COUNT) */
    u32 *d_tile_cnt = nullptr;
    u64 *d_start = nullptr, *d_seq = nullptr; /* the piece's records: n_start of them */
    u32 *d_wrap = nullptr;
    u16 *d_glen = nullptr;
    u64 n_start = 0, good = 0;
    u64 fig[DP_COUNT] = {0, 0, 0, 0, 0, 0, 0};
};

struct IngestFile {
    std::string path;
    int fd = -1;
    char last = 0;
    bool fastq = false;
    u64 n = 0; /* bytes of text */
    /* a BGZF file (map != null): n and the piece's text are its TEXT (known once the member chain is walked); the file itself is comp_n bytes at d_comp */
    const u8 *map = nullptr;
    u64 comp_n = 0;
    u8 *d_comp = nullptr;
    /* under a communicator: the member chain, walked by every rank, and the members [m_first, m_first + m_count) that hold the rank's piece */
    std::vector<infl::BgzfBlock> blocks;
    uint64_t m_first = 0, m_count = 0;
    IngestPiece p;
};
} // namespace

static void ingest_tables(FxTables *tb)
{
    memset(tb, 0, sizeof *tb);
    auto code = [](char ch) { return ch == 'A' ? 0ull : (ch == 'C' ? 1ull : (ch == 'G' ? 2ull : 3ull)); };
    tb->n_rep = (u32)DISCO_N_END_REPEATS;
    for (u32 r = 0; r < tb->n_rep; r++) {
        u64 v = 0;
        for (int x = 0; x < 29; x++) v = (v << 2) | code(kEndRepeats[r][x]);
        tb->rep58[r] = v;
    }
    tb->n_motif = (u32)DISCO_N_MOTIFS;
    for (u32 m = 0; m < tb->n_motif; m++) {
        const size_t l = strlen(kMotifs[m]);
        tb->motif_len[m] = (u8)l;
        for (size_t x = 0; x < l; x++) {
            tb->motif[m][x] = (u8)kMotifs[m][x];
            tb->need[m][code(kMotifs[m][x])]++;
        }
    }
    static_assert(DISCO_N_END_REPEATS <= FX_MAX_REPEATS && DISCO_N_MOTIFS <= FX_MAX_MOTIFS, "filter tables");
}

/* the file's bytes into d_text: host threads pread slices of a chunk into one half of a pinned ring while the other half travels */
/* flags of the pinned staging ring (DISCO_RING_MODE: 0 the runtime's default, 1 non-coherent = cached on the host side) */
static unsigned ring_alloc_flags()
{
    const int mode = env_int("DISCO_RING_MODE", 0);
    return mode == 1 ? hipHostMallocNonCoherent : (mode == 2 ? hipHostMallocCoherent : hipHostMallocDefault);
}

/* the context's pinned ring and its two events (first use), for what enters the device (ingest_ring: with the copy stream) and for
 * what leaves it (RingSink). Measured, round 5: calls into the runtime from this thread — this
 * allocation, every hipMemcpyAsync of the reader — can wait behind the helper thread's hipMalloc of the 28 GB hit buffer; that is the
 * stage's "slow mode" (files into HBM 0.2 s or, in bursts, 0.6-1.8 s with the reader's own waits unchanged). Making the ring first moves
 * the overlap onto the filter kernels instead (0.12 -> 0.18 s): no gain, not kept. */
static const size_t RING_HALF = 128u << 20;
static int pinned_ring(disco_ctx *c, const char *who)
{
    CHK(ring_back_from_rows(c));
    if (!c->h_ring) {
        if (hipHostMalloc(&c->h_ring, 2 * RING_HALF, ring_alloc_flags()) != hipSuccess) {
            c->h_ring = nullptr;
            (void)hipGetLastError();
            return fail(c, DISCO_E_NOMEM, "%s: no pinned staging memory", who);
        }
        c->ring_half = RING_HALF;
        for (int i = 0; i < 2; i++) HIPCHK(c, hipEventCreateWithFlags(&c->ev_ring[i], hipEventDisableTiming));
    }
    return DISCO_OK;
}
static int ingest_ring(disco_ctx *c)
{
    CHK(pinned_ring(c, "disco_ingest_fasta"));
    return ensure_copy_stream(c);
}

/* file_off: the bytes [file_off, file_off + n) of the file; own_ring: a pinned ring of the caller's (own_ring_bytes in all) instead of the context's */
static int ingest_read_file(disco_ctx *c, int fd, u64 n, u8 *d_text, unsigned threads, u64 file_off = 0, void *own_ring = nullptr, size_t own_ring_bytes = 0)
{
    /* The file travels through a pinned ring of RING_SLOTS slots (256 MB in all, as the two halves of rounds 3-4 were): reader threads
     * that live as long as the file — no thread is started per slot — pread piece after piece, in file order, into the next slot that is
     * free; the main thread sends a slot to the device as soon as its pieces are in, two copies in flight, and hands a slot back when its
     * copy is through. With two halves the readers waited for the copy of the half before last before they could start (0.8 of every
     * 3.3 ms: `waiting for the ring` in the DISCO_VERBOSE line of round 4); with four slots reading runs ahead of the link. */
    constexpr unsigned RING_SLOTS = 4;
    const size_t HALF = 128u << 20, SLOT = own_ring ? own_ring_bytes / RING_SLOTS : 2 * HALF / RING_SLOTS;
    if (own_ring) CHK(ensure_copy_stream(c));
    else CHK(ingest_ring(c));
    char *const h_ring = own_ring ? (char *)own_ring : (char *)c->h_ring;
    /* (the ring's slots need an event each: ev_ring has two, the upload's ev_copied — idle here — the others) */
    hipEvent_t ev[RING_SLOTS] = {own_ring ? c->ev_copied[2] : c->ev_ring[0], own_ring ? c->ev_unpacked[1] : c->ev_ring[1], c->ev_copied[0], c->ev_copied[1]};
    /* SIX readers whatever -t says (round 6; DISCO_INGEST_THREADS: measurement): the link, not the page cache, is what the file waits for, and
     * every reader beyond what keeps the ring full only competes with the DMA engine for the host's memory — 8.1 GB into HBM in 155-160 ms
     * with 5-6 readers, 195-280 ms with 16, 165-300 with 3-4 (16-core host of this pool, four runs each: profiles/r06_experiments.txt H) */
    threads = (unsigned)env_int("DISCO_INGEST_THREADS", (int)std::min(threads, 6u));
    threads = std::max(1u, std::min(threads, 64u));
    CHK(copy_stream_after_stream(c));
    const u64 n_chunks = (n + SLOT - 1) / SLOT;
    const u64 n_pieces = n_chunks * threads;
    std::atomic<u64> next_piece{0};
    std::vector<std::atomic<int>> slot_free(n_chunks), pieces_in(n_chunks); /* chunk k: its slot may be written / pieces of it that are in */
    for (u64 k = 0; k < n_chunks; k++) {
        slot_free[k].store(k < RING_SLOTS ? 1 : 0);
        pieces_in[k].store(0);
    }
    std::atomic<bool> ok{true}, stop{false};
    auto nap = [] { std::this_thread::sleep_for(std::chrono::microseconds(30)); };
    std::vector<std::thread> th;
    for (unsigned t = 0; t < threads; t++)
        th.emplace_back([&]() {
            for (;;) {
                const u64 p = next_piece.fetch_add(1);
                if (p >= n_pieces) return;
                const u64 k = p / threads;
                const unsigned piece = (unsigned)(p % threads);
                while (!slot_free[k].load(std::memory_order_acquire)) {
                    if (stop.load()) return;
                    nap();
                }
                const u64 off = k * (u64)SLOT;
                const size_t len = (size_t)std::min<u64>(SLOT, n - off);
                char *slot = h_ring + (k % RING_SLOTS) * SLOT;
                size_t p0 = len * piece / threads, p1 = len * (piece + 1) / threads;
                while (p0 < p1 && ok.load()) {
                    const ssize_t got = pread(fd, slot + p0, p1 - p0, (off_t)(file_off + off + p0));
                    if (got <= 0) {
                        ok.store(false);
                        break;
                    }
                    p0 += (size_t)got;
                }
                pieces_in[k].fetch_add(1, std::memory_order_release);
            }
        });
    struct Join { /* whatever happens below, the readers are told and waited for */
        std::vector<std::thread> &th;
        std::atomic<bool> &stop;
        ~Join()
        {
            stop.store(true);
            for (auto &x : th)
                if (x.joinable()) x.join();
        }
    } join_readers{th, stop};
    double t_fill = 0, t_copy = 0;
    const auto t_all = HClock::now();
    for (u64 k = 0; k < n_chunks; k++) {
        auto tw = HClock::now();
        while (pieces_in[k].load(std::memory_order_acquire) < (int)threads && ok.load()) nap();
        t_fill += ms_since(tw);
        if (!ok.load()) return fail(c, DISCO_E_ARG, "disco_ingest_fasta: read error");
        const u64 off = k * (u64)SLOT;
        const size_t len = (size_t)std::min<u64>(SLOT, n - off);
        HIPCHK(c, hipMemcpyAsync(d_text + off, h_ring + (k % RING_SLOTS) * SLOT, len, hipMemcpyHostToDevice, c->copy_stream));
        HIPCHK(c, hipEventRecord(ev[k % RING_SLOTS], c->copy_stream));
        tw = HClock::now();
        if (k >= 1) { /* the copy before this one: through, its slot goes back to the readers (this copy is queued behind it already) */
            HIPCHK(c, hipEventSynchronize(ev[(k - 1) % RING_SLOTS]));
            if (k - 1 + RING_SLOTS < n_chunks) slot_free[k - 1 + RING_SLOTS].store(1, std::memory_order_release);
        }
        t_copy += ms_since(tw);
    }
    auto tw = HClock::now();
    HIPCHK(c, hipStreamSynchronize(c->copy_stream));
    if (getenv("DISCO_VERBOSE"))
        fprintf(stderr, "[disco] file reader: %.1f MB in %llu slots of %zu MB, %u readers: waited %.1f ms for pieces, %.1f ms for copies, last copy %.1f ms, all %.1f ms\n", n / 1e6,
                (unsigned long long)n_chunks, SLOT >> 20, threads, t_fill, t_copy, ms_since(tw), ms_since(t_all));
    return DISCO_OK;
}

/* ---- BGZF: the members of a compressed file decoded on the device (kernel: disco_bgzf.h, decoder: disco_inflate.h) ------------------- */
/* one wavefront per member on the context's stream, waited for: the nb members blk[] — whose payloads lie at d_comp + in_off — write
 * what they hold of the window [win_lo, win_lo + win_n) of the file's text to d_text[0, win_n). d_blk: room for the member table,
 * d_status: a word per member and one more. *why = INFL_OK, or the error of member *bad OF THE LAUNCH, the first one the kernel did
 * not accept (its text is then not written) */
static int bgzf_inflate_run(disco_ctx *c, const u8 *d_comp, const infl::BgzfBlock *blk, u64 nb, infl::BgzfBlock *d_blk, u32 *d_status, u8 *d_text, u64 win_lo, u64 win_n, uint64_t *bad,
                            int *why)
{
    *why = infl::INFL_OK;
    *bad = 0;
    if (nb == 0 || nb >= (1ull << 31)) return fail(c, DISCO_E_ARG, "BGZF: %llu members out of range", (unsigned long long)nb);
    HIPCHK(c, hipMemcpyAsync(d_blk, blk, nb * sizeof(infl::BgzfBlock), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(d_status, 0, (nb + 1) * sizeof(u32), c->stream));
    BgzfArgs a;
    a.comp = d_comp;
    a.blk = d_blk;
    a.n_blk = (u32)nb;
    a.text = d_text;
    a.win_lo = win_lo;
    a.win_n = win_n;
    a.status = d_status;
    hipLaunchKernelGGL(bgzf_inflate_kernel, dim3((unsigned)nb), dim3(64), 0, c->stream, a);
    HIPCHK(c, hipGetLastError());
    u32 n_err = 0;
    HIPCHK(c, hipMemcpyAsync(&n_err, d_status + nb, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n_err) {
        std::vector<u32> st(nb);
        HIPCHK(c, hipMemcpy(st.data(), d_status, nb * sizeof(u32), hipMemcpyDeviceToHost));
        for (u64 k = 0; k < nb; k++)
            if (st[k]) {
                *bad = k;
                *why = (int)st[k];
                break;
            }
        if (*why == infl::INFL_OK) return fail(c, DISCO_E_STATE, "BGZF: %u members in error, none marked", n_err);
    }
    return DISCO_OK;
}

extern "C" int64_t disco_inflate_bgzf(disco_ctx *c, const void *bgzf, uint64_t n_bytes, void *out, uint64_t cap)
{
    DISCO_TRACE("disco_inflate_bgzf");
    if (!c || !bgzf) return c ? fail(c, DISCO_E_ARG, "disco_inflate_bgzf: null argument") : DISCO_E_ARG;
    std::vector<infl::BgzfBlock> blocks;
    uint64_t total = 0, bad = 0;
    if (const char *why = infl::bgzf_walk((const u8 *)bgzf, n_bytes, blocks, &total, &bad))
        return fail(c, DISCO_E_UNSUPPORTED, "disco_inflate_bgzf: member %llu: %s", (unsigned long long)bad, why);
    if (!out) return (int64_t)total;
    if (cap < total) return fail(c, DISCO_E_CAPACITY, "disco_inflate_bgzf: %llu bytes of text, room for %llu", (unsigned long long)total, (unsigned long long)cap);
    HIPCHK(c, hipSetDevice(c->device));
    LocalBuf<u8> d_comp(c), d_text(c);
    LocalBuf<infl::BgzfBlock> d_blk(c);
    LocalBuf<u32> d_status(c);
    int e = infl::INFL_OK;
    CHK(ensure(c, d_comp, n_bytes));
    CHK(ensure(c, d_text, total));
    CHK(ensure(c, d_blk, blocks.size()));
    CHK(ensure(c, d_status, blocks.size() + 1));
    HIPCHK(c, hipMemcpyAsync(d_comp.p, bgzf, n_bytes, hipMemcpyHostToDevice, c->stream));
    CHK(bgzf_inflate_run(c, d_comp, blocks.data(), blocks.size(), d_blk, d_status, d_text, 0, total, &bad, &e));
    if (e == infl::INFL_OK && total) HIPCHK(c, hipMemcpy(out, d_text.p, total, hipMemcpyDeviceToHost));
    if (e != infl::INFL_OK) return fail(c, DISCO_E_UNSUPPORTED, "disco_inflate_bgzf: member %llu: %s", (unsigned long long)bad, infl::reason(e));
    return (int64_t)total;
}

extern "C" int64_t disco_inflate_bgzf_window(disco_ctx *c, const void *bgzf, uint64_t n_bytes, uint64_t text_lo, uint64_t text_n, void *out)
{
    DISCO_TRACE("disco_inflate_bgzf_window");
    if (!c || !bgzf) return c ? fail(c, DISCO_E_ARG, "disco_inflate_bgzf_window: null argument") : DISCO_E_ARG;
    std::vector<infl::BgzfBlock> blocks, sub;
    uint64_t total = 0, bad = 0, first = 0, count = 0, comp_lo = 0, comp_n = 0;
    if (const char *why = infl::bgzf_walk((const u8 *)bgzf, n_bytes, blocks, &total, &bad))
        return fail(c, DISCO_E_UNSUPPORTED, "disco_inflate_bgzf_window: member %llu: %s", (unsigned long long)bad, why);
    const uint64_t n = text_lo < total ? std::min(text_n, total - text_lo) : 0;
    if (!out || n == 0) return (int64_t)n;
    infl::bgzf_window_members(blocks, text_lo, n, &first, &count);
    infl::bgzf_rebase(blocks, first, count, sub, &comp_lo, &comp_n);
    HIPCHK(c, hipSetDevice(c->device));
    LocalBuf<u8> d_comp(c), d_text(c);
    LocalBuf<infl::BgzfBlock> d_blk(c);
    LocalBuf<u32> d_status(c);
    int e = infl::INFL_OK;
    CHK(ensure(c, d_comp, comp_n));
    CHK(ensure(c, d_text, n));
    CHK(ensure(c, d_blk, sub.size()));
    CHK(ensure(c, d_status, sub.size() + 1));
    HIPCHK(c, hipMemcpyAsync(d_comp.p, (const u8 *)bgzf + comp_lo, comp_n, hipMemcpyHostToDevice, c->stream));
    CHK(bgzf_inflate_run(c, d_comp, sub.data(), sub.size(), d_blk, d_status, d_text, text_lo, n, &bad, &e));
    if (e == infl::INFL_OK) HIPCHK(c, hipMemcpy(out, d_text.p, n, hipMemcpyDeviceToHost));
    if (e != infl::INFL_OK) return fail(c, DISCO_E_UNSUPPORTED, "disco_inflate_bgzf_window: member %llu: %s", (unsigned long long)(first + bad), infl::reason(e));
    return (int64_t)n;
}

/* ---- the input stage as steps over one IngestJob, with two drivers: disco_ingest_fasta (below: one piece per file, no exchange) and
 * disco_dist_ingest_fasta (multi-GPU section: the pieces of the rank's share, all-gathers and an all-to-all between the steps). A step
 * answers DISCO_OK, an error it has recorded with fail, or INGEST_DECLINED with the reason left in the job (an input the HOST stage reads:
 * plain gzip, a '>' inside a line ...): only the drivers turn that into their message. Whatever the job holds goes with it, on every way out. */
extern "C++" { /* (the job's `get` is a template) */
namespace {
constexpr int INGEST_DECLINED = 1;
/* why the stage leaves a job to the host stage (the ranks of a communicator tell each other by code). One condition has two codes: a plain
 * file that cannot be opened is DR_NO_OPEN on one GPU and DR_UNREADABLE under a communicator — the words each entry point had before */
enum { DR_NONE = 0, DR_GZ, DR_GZ_MEMBER, DR_BGZF_MEMBER, DR_GZ_COMM, DR_NO_OPEN, DR_UNREADABLE, DR_FORM, DR_IRREGULAR, DR_NO_READ, DR_LONG_RECORD, DR_COUNT };
const char *const kIngestDecline[DR_COUNT] = {"", "gzip input", "gzip input,", "BGZF", /* (the last two: + "member N: ...", IngestJob::decline's detail) */
                                              "gzip input (a .gz name is the host stage's under a communicator)", "unreadable file", "empty or unreadable file", "neither FASTA nor FASTQ",
                                              "a '>' inside a line, an irregularly wrapped long record, or no record", "no good read (or more than 2^31)", "a record of 2^21 bytes or more"};

struct IngestJob {
    disco_ctx *c;
    const char *who; /* the entry point, for messages */
    unsigned threads; /* of the file reader */
    std::vector<IngestFile> F;
    u8 *arena = nullptr; /* the transient buffers (text, record arrays) are carved out of it, 256-byte aligned */
    u64 arena_cap = 0, arena_used = 0;
    std::vector<std::pair<void *, size_t>> owned; /* pieces that did not fit the arena: allocations of their own, in hbm_bytes */
    FxTables tb;
    u64 total_bytes = 0; /* text of all files as it will lie in HBM (a .gz name: an estimate) */
    float read_s = 0;
    int why_code = DR_NONE; /* of a decline: the code, the file's number, and both in words */
    size_t why_file = 0;
    std::string why, where;
    const HClock::time_point t_begin = HClock::now();
    IngestJob(disco_ctx *ctx, const char *entry, int n_files, uint32_t host_threads) : c(ctx), who(entry), threads(host_threads ? host_threads : 16u), F((size_t)n_files) { ingest_tables(&tb); }
    IngestJob(const IngestJob &) = delete;
    ~IngestJob()
    {
        for (auto &f : F) {
            if (f.map) munmap((void *)f.map, (size_t)f.comp_n);
            if (f.fd >= 0) close(f.fd);
        }
        for (auto &o : owned) {
            (void)hipFree(o.first);
            c->hbm_bytes -= o.second;
        }
    }
    float seconds() const { return ms_since(t_begin) * 1e-3f; }
    int decline(int code, const IngestFile &f, const char *detail = nullptr)
    {
        why_code = code, why_file = (size_t)(&f - F.data()), where = f.path;
        why = detail ? std::string(kIngestDecline[code]) + " " + detail : kIngestDecline[code];
        return INGEST_DECLINED;
    }
    template <typename T>
    int get(T **pp, u64 count) /* from the arena, or an allocation of its own */
    {
        const size_t bytes = std::max<u64>(count, 1) * sizeof(T), room = (bytes + 255) & ~(size_t)255;
        if (arena && arena_used + room <= arena_cap) {
            *pp = (T *)(arena + arena_used);
            arena_used += room;
            return DISCO_OK;
        }
        if (hipMalloc((void **)pp, bytes) != hipSuccess) {
            (void)hipGetLastError();
            return fail(c, DISCO_E_NOMEM, "disco_ingest_fasta: out of device memory");
        }
        c->hbm_bytes += bytes;
        owned.emplace_back((void *)*pp, bytes);
        return DISCO_OK;
    }
};

/* what the figures of all pieces fold into (ingest_fold) */
struct IngestFold {
    ReadShape shape{0, 0, 0, 0, 0, 0xFFFFu}; /* of the job's good reads */
    u64 total_records = 0, too_long = 0;
    std::vector<u64> share; /* rank g's good reads are the ids [share[g], share[g + 1]): shares follow each other in file order */
    std::vector<u64> file_id_base, file_rec_base; /* per file: first read id, records before the file (the context's ingest_id_base / ingest_rec_base once the table is begun) */
    std::vector<u64> id_base, rec_in_file, n_rec; /* per file, of THIS rank's piece: id of its first good read / records of the file in the pieces before / its records */
};
} // namespace
} // extern "C++"

/* whole tiles (16-byte loads) and aligned 8-byte words behind the end of a text of n bytes */
static u64 ingest_text_cap(u64 n) { return (n + FX_TILE + 63) / FX_TILE * FX_TILE + 64; }

/* a file opened and classified — regular, first byte '>' or '@'. Under a .gz name: BGZF only where the caller decodes it (may_bgzf: one
 * GPU, and the ranks of a communicator that were told to with DISCO_DIST_BGZF=1; plain gzip is one serial stream, the host stage's), a
 * decline otherwise. A BGZF file is mapped and left unclassified: its text is known once its members are. Answers a decline code */
static int ingest_open_file(IngestFile &f, const char *path, bool may_bgzf)
{
    f.path = path ? path : "";
    const bool gz_name = f.path.size() >= 3 && f.path.compare(f.path.size() - 3, 3, ".gz") == 0;
    if (gz_name && !may_bgzf) return DR_GZ_COMM;
    struct stat st;
    f.fd = open(f.path.c_str(), O_RDONLY);
    if (f.fd < 0 && !gz_name) return may_bgzf ? DR_NO_OPEN : DR_UNREADABLE; /* (the words each entry point has always had for it) */
    if (f.fd < 0 || fstat(f.fd, &st) != 0 || !S_ISREG(st.st_mode) || st.st_size < 1) return gz_name ? DR_GZ : DR_UNREADABLE;
    if (gz_name) {
        u32 hdr = 0, bsize = 0;
        void *m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, f.fd, 0); /* for the header walk only: the readers pread */
        if (m == MAP_FAILED) return DR_GZ;
        f.map = (const u8 *)m;
        f.comp_n = (u64)st.st_size;
        return infl::bgzf_header(f.map, f.comp_n, 0, &hdr, &bsize) ? DR_GZ : DR_NONE;
    }
    char first = 0;
    if (pread(f.fd, &first, 1, 0) != 1 || pread(f.fd, &f.last, 1, st.st_size - 1) != 1) return DR_UNREADABLE;
    if (first != '>' && first != '@') return DR_FORM;
    f.fastq = first == '@';
    f.n = (u64)st.st_size;
    return DR_NONE;
}

/* step (one GPU): the files, and the bytes their text will take in HBM */
static int ingest_open(IngestJob &j, const char *const *paths)
{
    for (size_t fi = 0; fi < j.F.size(); fi++) {
        IngestFile &f = j.F[fi];
        if (const int code = ingest_open_file(f, paths[fi], true)) return j.decline(code, f);
        /* BGZF: the text's size is known when the chain is walked, behind the transfer: the arena is sized for five times the file (FASTA
         * at level 6: four); a text that does not fit gets a piece of its own */
        j.total_bytes += f.map ? ((f.comp_n + 255) & ~255ull) + ingest_text_cap(f.comp_n * 5) : ingest_text_cap(f.n);
    }
    return DISCO_OK;
}

/* step: the arena. The transient buffers of this stage (text, record arrays) come out of ONE allocation. Where memory is plentiful it
 * is the stage's own (kept by the context: freeing 10 GB right before the pass made the pass's first allocations take 0.6 s), and the
 * hit buffer the probe will want — 64 candidate slots per read, 28 GB at 50 M reads, 0.5-0.9 s of hipMalloc — is allocated by a
 * thread of its own while the files travel to HBM and the filter runs (it may outlive this call: settle_hits_prealloc joins it). Where
 * it is not (2 x 10^8 reads on one GPU), the arena IS the hit buffer, as in round 3: the text lives where the candidates will. A
 * previous pass's results are gone either way. */
static int ingest_choose_arena(IngestJob &j)
{
    disco_ctx *c = j.c;
    if (c->phase > 1) c->phase = 1;
    c->d_adj = nullptr;
    c->adj_total = 0;
    settle_hits_prealloc(c);
    /* hit entries: 64 per read as the probe will ask, a chunk per resident wave; reads estimated at one per 150 bytes of text (shorter
     * records: the probe grows the buffer itself) */
    const u64 want = (j.total_bytes / 150) * 64 + (u64)c->n_cu * 32 * PR_CHUNK + (1u << 16);
    const u64 own_bytes = j.total_bytes + (j.total_bytes / 100) * 28 + (64ull << 20); /* text + record arrays (a record per 100 bytes at worst here; more: pieces of their own) */
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) return fail(c, DISCO_E_HIP, "disco_ingest_fasta: hipMemGetInfo failed");
    const u64 rest = (j.total_bytes / 150) * 200 + (4ull << 30); /* the read table and the index next to it */
    if (c->arena.base && !c->comm && c->arena.used == 0 && !c->d_ingest) { /* the last call's arena, idle again: this call's text goes there */
        /* (counted as one buffer again: the handover took it out of the sum) */
        adopt(c, c->d_ingest, DevBuf<u8>{(u8 *)c->arena.base, c->arena.size});
        c->arena = DevArena();
        c->hbm_peak = std::max(c->hbm_peak, c->hbm_bytes);
    }
    const bool split = !getenv("DISCO_INGEST_SHARED_ARENA") && !c->arena.base && (u64)fr + c->d_hits.cap * 8 + c->d_ingest.cap > std::max(want, c->d_hits.cap) * 8 + own_bytes + rest + (16ull << 30);
    if (split) {
        if (own_bytes > c->d_ingest.cap && ensure(c, c->d_ingest, own_bytes) != DISCO_OK) c->err.clear();
        if (want > c->d_hits.cap && c->d_ingest.cap) {
            /* the buffer at hand is too small for the probe and is not this call's arena: it goes now (should the thread's allocation fail,
             * the probe allocates its own, as on a fresh context), and what is asked for is counted now, not by the next call to join the thread */
            release(c, c->d_hits);
            c->hbm_bytes += (c->prealloc_asked = want) * 8;
            c->hits_prealloc = std::thread([c, dev = c->device, want]() {
                void *p = nullptr;
                if (hipSetDevice(dev) == hipSuccess && hipMalloc(&p, want * 8) == hipSuccess) c->prealloc = DevBuf<u64>{(u64 *)p, want};
                else (void)hipGetLastError();
            });
        }
    }
    if (split && c->d_ingest.cap) {
        j.arena = c->d_ingest;
        j.arena_cap = c->d_ingest.cap;
    } else {
        if (want > c->d_hits.cap && (u64)fr + c->d_hits.cap * 8 > want * 8 + rest && ensure(c, c->d_hits, want) != DISCO_OK) /* room for it next to the table and the index */
            c->err.clear();
        j.arena = (u8 *)c->d_hits.p;
        j.arena_cap = c->d_hits.cap * 8;
    }
    return DISCO_OK;
}

/* a BGZF file's text: the file into HBM while a host thread walks its member chain; then one wavefront per member writes the text */
static int ingest_text_bgzf(IngestJob &j, IngestFile &f)
{
    disco_ctx *c = j.c;
    const auto t_read = HClock::now();
    CHK(j.get(&f.d_comp, f.comp_n));
    std::vector<infl::BgzfBlock> blocks;
    uint64_t total = 0, bad = 0;
    const char *why = nullptr;
    float walk_ms = 0;
    std::thread walker([&]() {
        const auto t0 = HClock::now();
        why = infl::bgzf_walk(f.map, f.comp_n, blocks, &total, &bad);
        walk_ms = ms_since(t0);
    });
    const int rrc = ingest_read_file(c, f.fd, f.comp_n, f.d_comp, j.threads);
    walker.join();
    j.read_s += ms_since(t_read) * 1e-3f;
    CHK(rrc);
    char msg[160];
    if (why || total == 0) {
        snprintf(msg, sizeof msg, "member %llu: %s", (unsigned long long)bad, why ? why : "no text");
        return j.decline(DR_GZ_MEMBER, f, msg);
    }
    const auto t_inf = HClock::now();
    f.n = total;
    infl::BgzfBlock *d_blk = nullptr;
    u32 *d_status = nullptr;
    CHK(j.get(&f.p.d_text, ingest_text_cap(f.n)));
    CHK(j.get(&d_blk, blocks.size()));
    CHK(j.get(&d_status, blocks.size() + 1));
    HIPCHK(c, hipMemsetAsync(f.p.d_text + f.n, 0, ingest_text_cap(f.n) - f.n, c->stream));
    int e = infl::INFL_OK;
    CHK(bgzf_inflate_run(c, f.d_comp, blocks.data(), blocks.size(), d_blk, d_status, f.p.d_text, 0, f.n, &bad, &e));
    if (e != infl::INFL_OK) {
        snprintf(msg, sizeof msg, "member %llu: %s", (unsigned long long)bad, infl::reason(e));
        return j.decline(DR_BGZF_MEMBER, f, msg);
    }
    char first = 0;
    HIPCHK(c, hipMemcpy(&first, f.p.d_text, 1, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(&f.last, f.p.d_text + f.n - 1, 1, hipMemcpyDeviceToHost));
    if (getenv("DISCO_VERBOSE"))
        fprintf(stderr, "[disco] BGZF %s: %.1f MB in %llu members -> %.1f MB of text; header walk %.1f ms (behind the transfer), inflate %.1f ms\n", f.path.c_str(), f.comp_n / 1e6,
                (unsigned long long)blocks.size(), f.n / 1e6, walk_ms, ms_since(t_inf));
    if (first != '>' && first != '@') return j.decline(DR_FORM, f);
    f.fastq = first == '@';
    return DISCO_OK;
}

/* step: the bytes of a piece into HBM — the byte in front of it (own_lo = 1; none at the top of a file), the owned bytes and what follows
 * them up to p.n. ring: the caller's pinned ring instead of the context's */
static int ingest_piece_text(IngestJob &j, IngestFile &f, void *ring = nullptr, size_t ring_bytes = 0)
{
    disco_ctx *c = j.c;
    IngestPiece &p = f.p;
    const auto t_read = HClock::now();
    CHK(j.get(&p.d_text, ingest_text_cap(p.n)));
    HIPCHK(c, hipMemsetAsync(p.d_text + p.n, 0, ingest_text_cap(p.n) - p.n, c->stream));
    const int rc = ingest_read_file(c, f.fd, p.n, p.d_text, j.threads, p.p0 - p.own_lo, ring, ring_bytes);
    j.read_s += ms_since(t_read) * 1e-3f;
    return rc;
}

/* step (one GPU): one file's text into HBM, plain or BGZF — the piece that owns every byte, with nothing in front and nothing behind */
static int ingest_text(IngestJob &j, IngestFile &f)
{
    if (f.map) CHK(ingest_text_bgzf(j, f));
    IngestPiece &p = f.p;
    p.p0 = p.own_lo = 0;
    p.p1 = p.own_hi = p.n = f.n;
    p.to_eof = p.prefix_nl = true;
    p.last_nl = f.last == '\n';
    return f.map ? DISCO_OK : ingest_piece_text(j, f);
}

/* step: the record starts of a piece, placed. FASTQ: line0 = newlines of the file in front of the piece (a whole file: 0) */
static int ingest_place_starts(IngestJob &j, IngestFile &f, u64 line0)
{
    disco_ctx *c = j.c;
    IngestPiece &p = f.p;
    u64 rec0 = 0; /* FASTQ: the file's records that start in front of the piece */
    if (f.fastq) {
        /* the lines that BEGIN in the owned bytes: one at the first byte if a newline stands in front of it, one behind every owned
         * newline but the piece's last byte (that line is the next piece's, or nobody's at the end of the file: a last line without a
         * newline is a line). Line l of the file begins record l / 4 where l is a multiple of 4: the reference starts a record whenever
         * bytes are left (BG/Dataset.cpp:255-293) */
        const u64 first = p.prefix_nl ? line0 : line0 + 1, lines = (p.prefix_nl ? 1 : 0) + p.own_nl - (p.last_nl ? 1 : 0);
        rec0 = (first + 3) / 4;
        p.n_start = (lines && (first + lines - 1) / 4 + 1 > rec0) ? (first + lines - 1) / 4 + 1 - rec0 : 0;
    }
    if (p.n_start >= (1ull << 32)) return j.decline(DR_IRREGULAR, f);
    CHK(j.get(&p.d_start, p.n_start));
    if (f.fastq)
        hipLaunchKernelGGL(fx_lines_kernel, dim3((unsigned)p.tiles), dim3(256), 0, c->stream, (const u8 *)p.d_text, p.n, p.own_lo, p.own_hi, line0, (u32 *)nullptr, (const u64 *)p.d_tile_base,
                           p.d_start, rec0, p.n_start, p.d_ctr);
    else
        hipLaunchKernelGGL(fx_starts_kernel, dim3((unsigned)p.tiles), dim3(256), 0, c->stream, (const u8 *)p.d_text, p.n, p.own_lo, p.own_hi, (u32 *)nullptr, (const u64 *)p.d_tile_base, p.d_start,
                           p.d_ctr);
    HIPCHK(c, hipGetLastError());
    return DISCO_OK;
}

/* step: the record starts of a piece, counted — FASTA: the '>' that start a line, which are placed right away; FASTQ: the owned
 * newlines (a record is every fourth LINE of the file: ingest_place_starts, once the lines in front of the piece are known) */
static int ingest_count_starts(IngestJob &j, IngestFile &f)
{
    disco_ctx *c = j.c;
    IngestPiece &p = f.p;
    p.tiles = (p.n + FX_TILE - 1) / FX_TILE;
    CHK(j.get(&p.d_tile_base, p.tiles + 1));
    CHK(j.get(&p.d_tile_cnt, p.tiles));
    CHK(j.get(&p.d_ctr, (u64)FX_CTR_COUNT));
    HIPCHK(c, hipMemsetAsync(p.d_ctr, 0, FX_CTR_COUNT * sizeof(u64), c->stream));
    u64 total = 0;
    if (f.fastq)
        hipLaunchKernelGGL(fx_lines_kernel, dim3((unsigned)p.tiles), dim3(256), 0, c->stream, (const u8 *)p.d_text, p.n, p.own_lo, p.own_hi, (u64)0, p.d_tile_cnt, (const u64 *)nullptr,
                           (u64 *)nullptr, (u64)0, (u64)0, p.d_ctr);
    else
        hipLaunchKernelGGL(fx_starts_kernel, dim3((unsigned)p.tiles), dim3(256), 0, c->stream, (const u8 *)p.d_text, p.n, p.own_lo, p.own_hi, p.d_tile_cnt, (const u64 *)nullptr, (u64 *)nullptr,
                           p.d_ctr);
    CHK((scan_exclusive<u32, u64>(c, p.d_tile_cnt, p.tiles, p.d_tile_base, false, &total)));
    if (!f.fastq) {
        p.n_start = total;
        return ingest_place_starts(j, f, 0);
    }
    p.own_nl = total; /* the newlines from own_lo on: the owned ones where nothing follows the owned bytes, else the kernel has summed those */
    if (p.own_hi < p.n) {
        HIPCHK(c, hipMemcpyAsync(&p.own_nl, p.d_ctr + FX_CTR_OWN_NL, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return DISCO_OK;
}

/* step: clean + filter the records of a piece; what is left of them as the piece's figures */
static int ingest_filter_piece(IngestJob &j, IngestFile &f)
{
    disco_ctx *c = j.c;
    IngestPiece &p = f.p;
    u64 h[FX_CTR_COUNT] = {0};
    /* where the last owned record ends: the first record start behind the owned bytes, or the end of the file. A piece that ends its
     * buffer (a whole file) has nothing behind it: its counters are read once, with the filter's */
    if (p.own_hi < p.n || !p.n_start) {
        HIPCHK(c, hipMemcpyAsync(h, p.d_ctr, sizeof h, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (h[FX_CTR_BAD_GT]) return j.decline(DR_IRREGULAR, f);
    }
    p.fig[DP_STARTS] = p.n_start;
    if (!p.n_start) return DISCO_OK;
    u64 end = p.n;
    if (h[FX_CTR_NEXT_INV]) end = ~h[FX_CTR_NEXT_INV];
    else if (!p.to_eof) return j.decline(DR_LONG_RECORD, f);
    CHK(j.get(&p.d_seq, p.n_start));
    CHK(j.get(&p.d_glen, p.n_start));
    CHK(j.get(&p.d_wrap, p.n_start));
    /* (a '>' that is the file's very last byte is filtered as a record of no bases: never good, never counted — ingest_fold) */
    const FxFilterArgs fa{.text = p.d_text, .n = end, .start = p.d_start, .n_start = p.n_start, .n_rec = p.n_start, .min_overlap = c->prm.min_overlap, .fastq = f.fastq ? 1u : 0u,
                          .glen = p.d_glen, .seq_begin = p.d_seq, .wrap = p.d_wrap, .ctr = p.d_ctr};
    hipLaunchKernelGGL(fx_filter_kernel, dim3(flat_grid(c, p.n_start)), dim3(256), 0, c->stream, fa, j.tb);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h, p.d_ctr, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (h[FX_CTR_BAD_GT] || h[FX_CTR_MULTILINE]) return j.decline(DR_IRREGULAR, f);
    const int from[DP_COUNT] = {-1, FX_CTR_GOOD, FX_CTR_TOO_LONG, FX_CTR_MAX_LEN, FX_CTR_MIN_LEN_INV, FX_CTR_N_LONG, FX_CTR_SHORT_MAX}; /* (DP_STARTS: above) */
    for (int k = DP_GOOD; k < DP_COUNT; k++) p.fig[k] = h[from[k]];
    p.good = p.fig[DP_GOOD];
    return DISCO_OK;
}

/* this job's figures as they travel: a status word (the communicator's), then DP_COUNT figures per file */
static std::vector<u64> ingest_figures(const IngestJob &j, u64 status)
{
    std::vector<u64> v(1 + j.F.size() * DP_COUNT, status); /* (every other word is written below) */
    for (size_t fi = 0; fi < j.F.size(); fi++) memcpy(&v[1 + fi * DP_COUNT], j.F[fi].p.fig, sizeof j.F[fi].p.fig);
    return v;
}

/* the figures of every rank's pieces, all[rank][ingest_figures] (one GPU: world = 1) -> the job: the shape of its reads, the per-file
 * counts, the ids of every rank's share and where this rank's pieces lie in them. Every rank computes the same from the same numbers */
static int ingest_fold(IngestJob &j, const std::vector<u64> &all, size_t world, size_t rank, disco_ingest_file *files, IngestFold *o)
{
    const size_t F = j.F.size(), PR = 1 + F * DP_COUNT;
    auto fig = [&](size_t g, size_t fi, int what) { return all[g * PR + 1 + fi * DP_COUNT + (size_t)what]; };
    ReadShape &s = o->shape;
    o->share.assign(world + 1, 0);
    o->id_base = o->rec_in_file = o->n_rec = std::vector<u64>(F, 0);
    o->file_id_base = o->file_rec_base = std::vector<u64>(F + 1, 0);
    for (size_t fi = 0; fi < F; fi++) {
        u64 starts = 0, good = 0;
        size_t last_piece = 0; /* the rank that owns the file's last record start */
        for (size_t g = 0; g < world; g++) {
            starts += fig(g, fi, DP_STARTS);
            if (fig(g, fi, DP_STARTS)) last_piece = g;
        }
        if (starts == 0 || starts >= (1ull << 32)) return j.decline(DR_IRREGULAR, j.F[fi]);
        /* a '>' that is the very last byte starts nothing (the reference's next getline fails) unless it is the only one; it still
         * ends the sequence of the record before it (disco_amd/host/fastx.cpp) */
        const bool lone_gt = !j.F[fi].fastq && starts > 1 && j.F[fi].last == '>';
        u64 recs = 0;
        for (size_t g = 0; g < world; g++) {
            const u64 nr = fig(g, fi, DP_STARTS) - ((lone_gt && g == last_piece) ? 1 : 0);
            if (g == rank) {
                o->id_base[fi] = s.n + good;
                o->rec_in_file[fi] = recs;
                o->n_rec[fi] = nr;
            }
            recs += nr;
            const u64 gd = fig(g, fi, DP_GOOD);
            good += gd;
            o->share[g + 1] += gd;
            o->too_long += fig(g, fi, DP_TOO_LONG);
            if (gd) {
                s.longest = std::max(s.longest, (u32)fig(g, fi, DP_MAX_LEN));
                s.shortest = std::min(s.shortest, 0xFFFFu - (u32)fig(g, fi, DP_MIN_LEN_INV));
                s.n_long += fig(g, fi, DP_N_LONG);
                s.short_max = std::max(s.short_max, (u32)fig(g, fi, DP_SHORT_MAX));
            }
        }
        files[fi] = disco_ingest_file{.first_index = o->total_records + 1, .last_index = o->total_records + recs, .good = good, .bad = recs - good};
        o->total_records += recs;
        s.n += good;
        o->file_id_base[fi + 1] = s.n;
        o->file_rec_base[fi + 1] = o->total_records;
    }
    for (size_t g = 0; g < world; g++) o->share[g + 1] += o->share[g];
    if (s.n == 0 || s.n >= (1ull << 31)) return j.decline(DR_NO_READ, j.F[0]);
    s.stride = (std::max<u32>(1, (s.longest + 31) / 32) + 7u) & ~7u;
    return DISCO_OK;
}

/* step: the good reads of this job's pieces into the table the driver has begun, at their ids — lengths, record numbers within the
 * file, rows packed straight from the text (the short class's where the table has two classes of rows). Nothing waits for the device */
static int ingest_place_reads(IngestJob &j, const IngestFold &o)
{
    disco_ctx *c = j.c;
    c->ingest_id_base = o.file_id_base; /* (here, not in the fold: a declined job leaves the context what the fetch calls read) */
    c->ingest_rec_base = o.file_rec_base;
    u64 max_rec = 0;
    for (auto &f : j.F) max_rec = std::max(max_rec, f.p.n_start);
    u64 *d_pos = nullptr;
    u8 *d_flag = nullptr;
    CHK(j.get(&d_pos, max_rec + 1));
    CHK(j.get(&d_flag, max_rec));
    for (size_t fi = 0; fi < j.F.size(); fi++) {
        const IngestPiece &p = j.F[fi].p;
        const u64 nr = o.n_rec[fi], id_base = o.id_base[fi];
        if (!nr) continue;
        hipLaunchKernelGGL(fx_flags_kernel, dim3(flat_grid(c, nr)), dim3(256), 0, c->stream, (const u16 *)p.d_glen, nr, d_flag);
        u64 good = 0;
        CHK((scan_exclusive<u8, u64>(c, d_flag, nr, d_pos, false, &good)));
        if (good != p.good) return fail(c, DISCO_E_STATE, "%s: %llu good reads counted, %llu placed", j.who, (unsigned long long)p.good, (unsigned long long)good);
        if (id_base + good > o.shape.n) return fail(c, DISCO_E_STATE, "%s: ids beyond the job's reads", j.who);
        if (!good) continue;
        hipLaunchKernelGGL(fx_ids_kernel, dim3(flat_grid(c, nr)), dim3(256), 0, c->stream, (const u16 *)p.d_glen, (const u64 *)d_pos, nr, id_base, c->d_rec_of_read.p, c->d_len);
        hipLaunchKernelGGL(fx_pack_kernel, dim3(flat_grid(c, good * (u64)c->S)), dim3(256), 0, c->stream, (const u8 *)p.d_text, (const u64 *)p.d_seq, (const u32 *)p.d_wrap,
                           (const u32 *)c->d_rec_of_read.p, (const u16 *)c->d_len, id_base, good, c->S, c->two_class ? (u32)DISCO_SHORT_MAX : 0xFFFFu, c->d_reads);
        if (o.rec_in_file[fi])
            hipLaunchKernelGGL(fx_rec_add_kernel, dim3(flat_grid(c, good)), dim3(256), 0, c->stream, c->d_rec_of_read.p, id_base, id_base + good, (u32)o.rec_in_file[fi]);
        HIPCHK(c, hipGetLastError());
    }
    return DISCO_OK;
}

/* step (one GPU): the read table — every file's reads in file order, then the long class's rows where the table has two classes */
static int ingest_build_table(IngestJob &j, const IngestFold &o)
{
    disco_ctx *c = j.c;
    const ReadShape &s = o.shape;
    CHK(begin_read_table(c, s, true)); /* (true: the arena may be the hit buffer) */
    CHK(ensure(c, c->d_rec_of_read, s.n));
    CHK(ingest_place_reads(j, o));
    if (c->two_class) { /* every read has its id and length: number the long ones, then their full and tail rows, file by file */
        u64 counted = 0;
        CHK(number_long_reads(c, c->d_ovf, c->d_long_ids, &counted));
        if (counted != s.n_long) return fail(c, DISCO_E_STATE, "disco_ingest_fasta: %llu long reads counted, %llu placed", (unsigned long long)s.n_long, (unsigned long long)counted);
        for (size_t fi = 0; fi < j.F.size(); fi++) {
            const IngestPiece &p = j.F[fi].p;
            if (!p.good) continue;
            hipLaunchKernelGGL(fx_pack_long_kernel, dim3(flat_grid(c, s.n_long * ((u64)s.stride + 8))), dim3(256), 0, c->stream, (const u8 *)p.d_text, (const u64 *)p.d_seq, (const u32 *)p.d_wrap,
                               (const u32 *)c->d_rec_of_read, (const u16 *)c->d_len, c->ingest_id_base[fi], p.good, (const u32 *)c->d_long_ids, s.n_long, s.n, (int)s.stride, c->tailb, c->d_full,
                               c->d_reads);
        }
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DISCO_OK;
}

/* step: the stage's own arena is free space from here on — the context's allocator serves the pass from it (its index, headers,
 * adjacency and result buffers: a dozen device allocations of 5-10 ms each that the first pass of a fresh context otherwise waits for) */
static void ingest_hand_over_arena(IngestJob &j)
{
    disco_ctx *c = j.c;
    if (!c->d_ingest || j.arena != c->d_ingest.p || getenv("DISCO_NO_ARENA_HANDOVER")) return;
    c->arena = DevArena();
    c->arena.free_at[0] = c->arena.size = c->d_ingest.cap & ~(u64)255;
    /* what the allocator serves out of it is counted buffer by buffer (dev_alloc): the arena itself leaves the sum, or every byte of
     * it would count twice in hbm_bytes / hbm_peak */
    c->arena.base = (char *)disown(c, c->d_ingest);
}

extern "C" int disco_ingest_fasta(disco_ctx *c, const char *const *paths, int n_files, uint32_t host_threads, disco_ingest_info *info, disco_ingest_file *files)
{
    DISCO_TRACE("disco_ingest_fasta");
    if (!c || !paths || n_files < 1 || !info || !files) return c ? fail(c, DISCO_E_ARG, "disco_ingest_fasta: null argument") : DISCO_E_ARG;
    if (c->comm) return fail(c, DISCO_E_UNSUPPORTED, "disco_ingest_fasta: single-GPU contexts only");
    HIPCHK(c, hipSetDevice(c->device));
    IngestJob job(c, "disco_ingest_fasta", n_files, host_threads);
    IngestFold o;
    int rc = ingest_open(job, paths);
    if (rc == DISCO_OK) rc = ingest_choose_arena(job);
    const float t_arena = job.seconds();
    for (int fi = 0; fi < n_files && rc == DISCO_OK; fi++) { /* every file, as one piece: its text into HBM, its records, clean + filter */
        IngestFile &f = job.F[(size_t)fi];
        rc = ingest_text(job, f);
        if (rc == DISCO_OK) rc = ingest_count_starts(job, f);
        if (rc == DISCO_OK && f.fastq) rc = ingest_place_starts(job, f, 0);
        if (rc == DISCO_OK) rc = ingest_filter_piece(job, f);
    }
    if (rc == DISCO_OK) rc = ingest_fold(job, ingest_figures(job, 0), 1, 0, files, &o);
    const float t_filtered = job.seconds();
    if (rc == DISCO_OK) rc = ingest_build_table(job, o);
    if (rc == INGEST_DECLINED) return fail(c, DISCO_E_UNSUPPORTED, "disco_ingest_fasta: %s (%s): the host input stage takes this job", job.why.c_str(), job.where.c_str());
    CHK(rc);
    if (getenv("DISCO_VERBOSE"))
        fprintf(stderr, "[disco] input stage: arena of %.1f GB %.3f s, files + records + filter %.3f s (files %.3f), table + ids + rows %.3f s\n", job.arena_cap / 1e9, t_arena,
                t_filtered - t_arena, job.read_s, job.seconds() - t_filtered);
    ingest_hand_over_arena(job);
    const ReadShape &s = o.shape;
    c->ingest_n = s.n;
    c->h_len_ok = false;
    c->phase = 1;
    *info = disco_ingest_info{.n_reads = s.n, .total_records = o.total_records, .too_long = o.too_long, .stride_words = std::max<u32>(1, (s.longest + 31) / 32),
                              .shortest = s.shortest, .longest = s.longest, .read_s = job.read_s, .device_s = job.seconds() - job.read_s};
    return DISCO_OK;
}

/* lengths and file indices of the reads [lo, hi) of a table the input stage made, to len[0 ..) and file_index[0 ..): a read's record
 * number within its file -> the 1-based number of the record among all records of the job */
static int ingest_fetch_range(disco_ctx *c, u64 lo, u64 hi, hipStream_t st, uint16_t *len, uint64_t *file_index)
{
    if (hi <= lo) return DISCO_OK;
    const u64 n = hi - lo;
    std::unique_ptr<u32[]> rec(new u32[n]);
    HIPCHK(c, hipMemcpyAsync(len, c->d_len + lo, n * 2, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(rec.get(), c->d_rec_of_read.p + lo, n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    const u32 *r = rec.get();
    for (size_t fi = 0; fi + 1 < c->ingest_id_base.size(); fi++) {
        const u64 a = std::max(lo, c->ingest_id_base[fi]), b = std::min(hi, c->ingest_id_base[fi + 1]), rb = c->ingest_rec_base[fi];
        if (b > a)
            parallel_for(b - a, [&, a, rb](u64 x, u64 y) {
                for (u64 i = a + x; i < a + y; i++) file_index[i - lo] = rb + (u64)r[i - lo] + 1; /* BG/Dataset.cpp:294: every record counts */
            });
    }
    return DISCO_OK;
}

extern "C" int disco_ingest_fetch(disco_ctx *c, uint16_t *len, uint64_t *file_index)
{
    if (!c || !len || !file_index) return c ? fail(c, DISCO_E_ARG, "disco_ingest_fetch: null argument") : DISCO_E_ARG;
    if (c->phase < 1 || c->ingest_n == 0 || c->ingest_n != c->n) return fail(c, DISCO_E_STATE, "disco_ingest_fetch: the reads of the context did not come from disco_ingest_fasta");
    HIPCHK(c, hipSetDevice(c->device));
    const u64 n = c->n;
    /* on the copy stream: the call may run on a host thread of its own while the context's stream is busy with the pass (buildG does
     * that: the per-read arrays are only needed by the writers) */
    CHK(ingest_fetch_range(c, 0, n, c->copy_stream ? c->copy_stream : c->stream, len, file_index));
    {
        std::lock_guard<std::mutex> lk(c->h_len_mu);
        if (!(c->h_len_ok && c->h_len.size() == n)) { /* (ensure_host_len may have mirrored them meanwhile) */
            if (c->h_len.size() != n) c->h_len.resize(n);
            uint16_t *hl = c->h_len.data();
            parallel_for(n, [&, hl](u64 b, u64 e_) { memcpy(hl + b, len + b, (e_ - b) * 2); });
            c->h_len_ok = true;
        }
    }
    return DISCO_OK;
}

int disco_adopt_reads(disco_ctx *c, const void *d_packed, uint32_t stride_words, const void *d_len, uint64_t n)
{
    if (!c || (n && (!d_packed || !d_len))) return c ? fail(c, DISCO_E_ARG, "disco_adopt_reads: null argument") : DISCO_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    CHK(set_reads_common(c, n, stride_words));
    c->d_reads = (u64 *)d_packed;
    c->d_len = (u16 *)d_len;
    c->reads_owned = false;
    return validate_reads(c);
}

/* the generator's spec as its kernel takes it, checked, and the stride of the table it fills (words; 64-byte rows) */
static int gen_spec(disco_ctx *c, const char *who, const disco_genspec_abi *s, disco_genspec *g, uint32_t *stride)
{
    memcpy(g, s, sizeof *g);
    const uint32_t longest = std::max<uint32_t>(s->len_max, DISCO_GEN_LONG_SHARE(g) ? DISCO_GEN_LONG_LEN(g) : 0u);
    if (s->len_min == 0 || s->len_max < s->len_min || longest > 32767 || s->n_contigs == 0 || s->contig_len < longest) return fail(c, DISCO_E_ARG, "%s: bad spec", who);
    *stride = (((longest + 31) / 32) + 7u) & ~7u;
    return DISCO_OK;
}

int disco_generate_reads(disco_ctx *c, const disco_genspec_abi *s)
{
    DISCO_TRACE("disco_generate_reads");
    if (!c || !s) return c ? fail(c, DISCO_E_ARG, "disco_generate_reads: null argument") : DISCO_E_ARG;
    disco_genspec g;
    ReadShape shape; /* (one stride here: a tail of long reads is converted at the index build, after whatever edits the table) */
    CHK(gen_spec(c, "disco_generate_reads", s, &g, &shape.stride));
    HIPCHK(c, hipSetDevice(c->device));
    shape.n = s->n_reads;
    CHK(begin_read_table(c, shape));
    if (c->n) hipLaunchKernelGGL(generate_reads_kernel, dim3(flat_grid(c, c->n * shape.stride)), dim3(256), 0, c->stream, g, c->d_reads, c->d_len, (int)shape.stride, (u64)0, c->n);
    HIPCHK(c, hipGetLastError());
    return validate_reads(c);
}

int disco_substitute_bases(disco_ctx *c, uint64_t seed, uint32_t rate_ppm)
{
    if (!c) return DISCO_E_ARG;
    if (c->phase != 1) return fail(c, DISCO_E_STATE, "disco_substitute_bases: call after the reads are set and before disco_build_index");
    if (rate_ppm > 1000000) return fail(c, DISCO_E_ARG, "disco_substitute_bases: rate above 10^6 ppm");
    if (c->two_class) /* (uploaded / ingested with a tail of long reads: head, tail and full rows would have to change together) */
        return fail(c, DISCO_E_UNSUPPORTED, "disco_substitute_bases: the table has two classes of rows (reads of more than 256 bases next to short ones); substitute "
                                            "into generated reads, or set DISCO_NO_TWO_CLASS=1");
    HIPCHK(c, hipSetDevice(c->device));
    const u64 lo = c->comm ? c->q_lo : 0, hi = c->comm ? c->q_hi : c->n; /* multi-GPU flow: the other ranks' rows arrive by all-gather */
    if (hi > lo && rate_ppm)
        hipLaunchKernelGGL(substitute_bases_kernel, dim3(flat_grid(c, (hi - lo) * (u64)c->S)), dim3(256), 0, c->stream, (u64)seed, rate_ppm, c->d_reads, c->d_len, c->S, lo, hi);
    c->index_counted = c->order_counted = c->order_ready = false; /* what an upload counted ahead was counted on the reads as they were */
    HIPCHK(c, hipGetLastError());
    return DISCO_OK;
}

int disco_download_reads(disco_ctx *c, uint64_t *packed, uint16_t *len)
{
    if (!c || c->phase < 1) return c ? fail(c, DISCO_E_STATE, "no reads") : DISCO_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    LocalBuf<u64> joined(c);
    if (packed && c->n && c->two_class) { /* the table as the caller knows it: one stride */
        CHK(ensure(c, joined, c->n * (u64)c->S_ext));
        hipLaunchKernelGGL(class_join_kernel, dim3(flat_grid(c, c->n * (u64)c->S_ext)), dim3(256), 0, c->stream, (const u64 *)c->d_reads, (const u64 *)c->d_full, c->S_ext,
                           (const u16 *)c->d_len, (const u32 *)c->d_ovf, c->n, joined);
        (void)hipMemcpyAsync(packed, joined, c->n * (u64)c->S_ext * 8, hipMemcpyDeviceToHost, c->stream);
    } else if (packed && c->n)
        HIPCHK(c, hipMemcpyAsync(packed, c->d_reads, c->n * (u64)c->S * 8, hipMemcpyDeviceToHost, c->stream));
    if (len && c->n) (void)hipMemcpyAsync(len, c->d_len, c->n * 2, hipMemcpyDeviceToHost, c->stream);
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, DISCO_E_HIP, "disco_download_reads: %s", hipGetErrorString(e));
    return DISCO_OK;
}

uint32_t disco_stride_words(const disco_ctx *c) { return c ? (uint32_t)(c->two_class ? c->S_ext : c->S) : 0; }
uint64_t disco_num_reads(const disco_ctx *c) { return c ? c->n : 0; }
uint64_t disco_long_rows(const disco_ctx *c) { return c && c->two_class ? c->n_long : 0; }

int disco_set_query_range(disco_ctx *c, uint64_t lo, uint64_t hi)
{
    if (!c) return DISCO_E_ARG;
    if (c->phase < 1 || c->phase > 2) return fail(c, DISCO_E_STATE, "disco_set_query_range: call after the reads are set and before disco_probe");
    if (lo > hi || hi > c->n) return fail(c, DISCO_E_ARG, "query range [%llu,%llu) outside [0,%llu)", (unsigned long long)lo, (unsigned long long)hi, (unsigned long long)c->n);
    c->q_lo = lo;
    c->q_hi = hi;
    return DISCO_OK;
}

/* ---------------------------------------------------------------------------------------------------------------- */
/* one stride -> two classes of rows (disco_kernels.h), at the first index build over the table: everything that edits a table (the
 * generator's substitutions) has been and gone by then. The decision is the device's own count of the long reads; the table that is
 * given up goes back to the allocator. */
static int two_class_convert(disco_ctx *c)
{
    if (c->two_class || !c->n || c->max_len <= (u32)DISCO_SHORT_MAX || !two_class_ok(c, c->S, c->n, 1, (u32)c->k + 1)) return DISCO_OK; /* (cheap part first) */
    const int Sx = c->S;
    LocalBuf<u32> ovf(c);
    CHK(ensure(c, ovf, c->n_alloc));
    CHK(zero_counter(c, CTR_SHORT_MAX));
    u64 n_long = 0;
    CHK(number_long_reads(c, ovf, nullptr, &n_long)); /* (class_split_kernel writes the ids) */
    CHK(read_counters(c));
    const u32 short_max = (u32)c->h_ctr[CTR_SHORT_MAX];
    if (!two_class_ok(c, Sx, c->n, n_long, short_max)) return DISCO_OK;
    LocalBuf<u64> rows8(c);
    ovf.give(c->d_ovf); /* (the context's from here on: released with the long class, also when something below fails) */
    int rca = ensure(c, rows8, (c->n + n_long) * 8);
    if (rca == DISCO_OK) rca = two_class_alloc(c, n_long, Sx, short_max);
    if (rca != DISCO_OK) { /* the table keeps its one stride */
        free_long_class(c);
        return rca;
    }
    hipLaunchKernelGGL(class_split_kernel, dim3(flat_grid(c, c->n * 8)), dim3(256), 0, c->stream, (const u64 *)c->reads_own, Sx, (const u16 *)c->d_len, (const u32 *)c->d_ovf, c->n, c->tailb,
                       rows8.p, c->d_full, c->d_long_ids);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream)); /* (the old table goes back: nothing of it may still be in flight) */
    rows8.give(c->reads_own);
    c->d_reads = c->reads_own;
    set_read_lengths(c, c->max_len, short_max, c->min_len);
    return DISCO_OK;
}

int disco_build_index(disco_ctx *c)
{
    DISCO_TRACE("disco_build_index");
    if (!c) return DISCO_E_ARG;
    if (c->phase < 1) return fail(c, DISCO_E_STATE, "disco_build_index: no reads");
    HIPCHK(c, hipSetDevice(c->device));
    ph_begin(c, DISCO_PH_INDEX);
    if (c->index_counted) { /* disco_upload_reads counted while it copied: the bucket counts, records, runs and keys are in place */
        c->index_counted = false;
    } else {
        CHK(two_class_convert(c));
        CHK(index_begin(c));
        const DiscoView v = view(c);
        IndexCountPlan pl;
        CHK(index_count_plan(c, v, 0, c->n, &pl));
        CHK(index_count_chunk(c, v, pl, index_rec_out(c), 0, c->n));
        if (c->two_class) CHK(index_count_long(c, v, pl, index_rec_out(c), pl.oslot, 0, c->n_long));
    }
    const bool binned = c->binned_index; /* (index_begin's decision, whoever counted) */
    if (!binned) CHK((scan_exclusive<u32, u32>(c, c->d_bkt, c->T + 1, c->d_bkt, false, nullptr)));
    /* the grouping of the reads (the processing order of probe / verify / selection / marking) was counted inside the index pass: it is
     * finished here, so that the fill can walk it (index_fill_ordered_kernel); disco_probe finds it ready */
    c->order_ready = false;
    if (c->order_counted && c->order_counted_lo == 0 && c->order_counted_hi == c->n && !c->two_class && !getenv("DISCO_NO_ORDERED_FILL")) {
        const u64 order_buckets = 1ull << c->order_counted_bits;
        CHK(ensure(c, c->d_order_own, c->n));
        ph_end(c, DISCO_PH_INDEX);
        ph_begin(c, DISCO_PH_ORDER);
        if (c->order_items) CHK(binned_build_order(c));
        else {
            CHK((scan_exclusive<u32, u32>(c, c->d_ocnt, order_buckets + 1, c->d_ocnt, false, nullptr)));
            hipLaunchKernelGGL(order_scatter_kernel, dim3(flat_grid(c, c->n)), dim3(256), 0, c->stream, c->d_okey, c->d_oslot, c->d_ocnt, 32u - (u32)c->order_counted_bits, (u64)0, c->n, c->d_len, c->d_order_own);
        }
        ph_end(c, DISCO_PH_ORDER);
        ph_begin(c, DISCO_PH_INDEX2);
        if (binned) CHK(binned_build_index(c)); /* (streams the records: no use for the order) */
        else hipLaunchKernelGGL(index_fill_ordered_kernel, dim3(flat_grid(c, c->n)), dim3(256), 0, c->stream, c->n, (const u64 *)c->d_order_own, (const ulonglong2 *)c->d_rec, (const u32 *)c->d_bkt, c->d_ent);
        ph_end(c, DISCO_PH_INDEX2);
        HIPCHK(c, hipGetLastError());
        c->order_ready = true;
        c->phase = 2;
        return DISCO_OK;
    }
    if (binned) CHK(binned_build_index(c));
    else if (c->n) hipLaunchKernelGGL(index_fill_kernel, dim3(flat_grid(c, 2 * c->n)), dim3(256), 0, c->stream, 2 * c->n, c->d_rec, c->d_bkt, c->d_ent);
    HIPCHK(c, hipGetLastError());
    ph_end(c, DISCO_PH_INDEX);
    c->phase = 2;
    return DISCO_OK;
}

/* ---------------------------------------------------------------------------------------------------------------- */
int disco_probe(disco_ctx *c)
{
    DISCO_TRACE("disco_probe");
    if (!c) return DISCO_E_ARG;
    if (c->phase < 2) return fail(c, DISCO_E_STATE, "disco_probe: build the index first");
    HIPCHK(c, hipSetDevice(c->device));
    CHK(settle_contained_rows(c)); /* rows of the previous pass still travelling read best[] */
    CHK(settle_keys(c));           /* ... and so does a key exchange that runs behind a multi-GPU pass */
    drop_edge_records(c);          /* prepared records are those of the previous pass */
    drop_contained_records(c);
    settle_hits_prealloc(c);
    const u64 nq = c->q_hi - c->q_lo;
    CHK(ensure(c, c->d_best, c->n_alloc));
    CHK(ensure(c, c->d_row_start, c->n));
    CHK(ensure(c, c->d_row_cnt, c->n));
    if (c->n_alloc) hipLaunchKernelGGL(fill_u64_kernel, dim3(flat_grid(c, c->n_alloc)), dim3(256), 0, c->stream, c->d_best, c->n_alloc, DISCO_NOKEY);
    HIPCHK(c, hipMemsetAsync(c->d_row_cnt, 0, std::max<u64>(c->n, 1) * sizeof(u32), c->stream));
    /* the index pass left the minimizer runs of the whole query range: probe_runs_kernel (several reads per wavefront, starts at the
     * bucket lookups); probe_kernel then only does the reads it is handed (unusable run lists, rows that outgrew their chunk) */
    const bool use_runs = c->runs_lpr != 0 && c->d_runs && c->q_lo >= c->runs_lo && c->q_hi <= c->runs_lo + c->runs_n;
    const ProbeKernel range_kernel = probe_pick(c, 0, use_runs);
    const int grid = range_kernel.runs ? wq_grid(c, range_kernel.runs, nq, "DISCO_PROBE_WAVES") : wq_grid(c, range_kernel.plain, nq, "DISCO_PROBE_WAVES");
    auto launch_probe = [&](const ProbeArgs &a, const ProbeKernel &k, int g) {
        if (k.runs) hipLaunchKernelGGL(k.runs, dim3(g), dim3(64), 0, c->stream, a, (const u32 *)c->d_runs, c->runs_by_pos ? ~0ull : c->runs_lo);
        else hipLaunchKernelGGL(k.plain, dim3(g), dim3(64), 0, c->stream, a);
    };
    const u64 chunk_slots = use_runs ? PR_CHUNK : PROBE_CHUNK;
    u64 want_hits = nq * 64 + (u64)grid * chunk_slots + (1u << 16);
    u32 want_slow = use_runs ? (u32)std::min<u64>(nq, nq / 64 + 1024 + (c->two_class ? c->n_long : 0)) : 1u;
    u32 want_big = (u32)std::min<u64>(nq, nq / 64 + 1024);
    for (int attempt = 0; attempt < 8; attempt++) {
        if (want_hits > c->d_hits.cap) {
            release(c, c->d_hits);
            size_t fr = 0, tot = 0;
            HIPCHK(c, hipMemGetInfo(&fr, &tot));
            if (want_hits * 8 > fr) {
                u64 can = fr / 8 / 10 * 9;
                if (can < (u64)grid * chunk_slots * 2) return fail(c, DISCO_E_NOMEM, "disco_probe: not enough HBM for the hit buffer (%llu entries wanted)", (unsigned long long)want_hits);
                want_hits = can;
            }
            CHK(ensure(c, c->d_hits, want_hits));
        }
        if (want_slow > c->d_slow_list.cap) CHK(ensure(c, c->d_slow_list, want_slow));
        CHK(grow_big_lists(c, want_big));
        HIPCHK(c, hipMemsetAsync(c->d_bump, 0, sizeof(u64), c->stream));
        HIPCHK(c, hipMemsetAsync(c->d_n_big, 0, sizeof(u32), c->stream));
        HIPCHK(c, hipMemsetAsync(c->d_n_slow, 0, sizeof(u32), c->stream));
        HIPCHK(c, hipMemsetAsync(c->d_ctr + CTR_KMER_HITS, 0, sizeof(u64) * 4, c->stream)); /* KMER_HITS, RAW_HITS, HITS_NEEDED, OVERFLOW */
        CHK(zero_counter(c, CTR_MAX_ROW));
        CHK(zero_counter(c, CTR_ES_BIG));
        CHK(zero_counter(c, CTR_ES_MID));
        c->es_big_counted = c->tr_big_counted = false;
        ProbeArgs a;
        a.v = view(c);
        a.hits = c->d_hits;
        a.row_start = c->d_row_start;
        a.row_cnt = c->d_row_cnt;
        c->h_probe_rare.bump = c->d_bump;
        c->h_probe_rare.hits_cap = c->d_hits.cap;
        c->h_probe_rare.big_list = c->d_big_list;
        c->h_probe_rare.big_cnt = c->d_big_cnt;
        c->h_probe_rare.n_big = c->d_n_big;
        c->h_probe_rare.big_cap = c->d_big_list.cap;
        c->h_probe_rare.slow_cap = c->d_slow_list.cap;
        c->h_probe_rare.slow_list = c->d_slow_list;
        c->h_probe_rare.n_slow = c->d_n_slow;
        c->h_probe_rare.ctr = c->d_ctr;
        CHK(ensure(c, c->d_probe_rare, 1));
        HIPCHK(c, hipMemcpyAsync(c->d_probe_rare, &c->h_probe_rare, sizeof(ProbeRare), hipMemcpyHostToDevice, c->stream));
        a.rare = c->d_probe_rare;
        CHK(ensure(c, c->d_meta_ord, std::max<u64>(nq, 1)));
        a.meta_ord = c->d_meta_ord;
        /* grouping of the query range by read-level minimizer for the probe and verify passes (DISCO_NO_ORDER=1: file order) */
        int order_bits = 16;
        const bool own_order = own_order_wanted(c, nq, &order_bits);
        a.order = nullptr;
        const u64 order_buckets = 1ull << order_bits;
        /* the index pass counted already (once: a retry of this loop finds the counters scanned and counts again) */
        /* (counted as items: no counts or slots to go on from — disco_build_index has finished that grouping, or it is made here) */
        const bool counted = c->order_counted && c->order_counted_lo == c->q_lo && c->order_counted_hi == c->q_hi && c->order_counted_bits == order_bits &&
                             (!c->order_items || c->order_ready);
        c->order_counted = false;
        if (c->loci) { /* the own list IS the processing order (grouped when the reads were dealt: dist_build_index) */
            c->d_order_used = c->d_order_own;
        } else if (own_order && c->order_ready && counted) { /* disco_build_index finished the grouping (its fill walks the order) */
            c->d_order_used = c->d_order_own; /* (DISCO_PH_ORDER was timed there) */
        } else if (own_order) {
            CHK(ensure(c, c->d_ocnt, order_buckets + 1));
            CHK(ensure(c, c->d_oslot, nq));
            CHK(ensure(c, c->d_order_own, nq));
            /* keys -> counts (+ slots) -> starts -> order */
            const u32 oshift = 32u - (u32)order_bits;
            ph_begin(c, DISCO_PH_ORDER);
            if (!counted) {
                HIPCHK(c, hipMemsetAsync(c->d_ocnt, 0, (order_buckets + 1) * sizeof(u32), c->stream));
                hipLaunchKernelGGL(order_count_kernel, dim3(flat_grid(c, nq)), dim3(256), 0, c->stream, c->d_okey + c->q_lo, nq, oshift, c->d_ocnt, c->d_oslot);
            }
            CHK((scan_exclusive<u32, u32>(c, c->d_ocnt, order_buckets + 1, c->d_ocnt, false, nullptr)));
            hipLaunchKernelGGL(order_scatter_kernel, dim3(flat_grid(c, nq)), dim3(256), 0, c->stream, c->d_okey + c->q_lo, c->d_oslot, c->d_ocnt, oshift, c->q_lo, nq, c->d_len, c->d_order_own);
            ph_end(c, DISCO_PH_ORDER);
            HIPCHK(c, hipGetLastError());
            c->d_order_used = c->d_order_own;
        } else if (c->order_external && nq) {
            CHK(ensure(c, c->d_order_own, nq));
            hipLaunchKernelGGL(order_pack_kernel, dim3(flat_grid(c, nq)), dim3(256), 0, c->stream, c->d_order, nq, c->d_len, c->d_order_own);
            HIPCHK(c, hipGetLastError());
            c->d_order_used = c->d_order_own;
        } else
            c->d_order_used = nullptr;
        a.order = c->d_order_used;
        c->order_q_lo = c->q_lo; /* (the range the order in d_order_used belongs to: later phases of the pass walk it too) */
        c->order_q_hi = c->q_hi;
        ph_begin(c, DISCO_PH_PROBE_KERNEL);
        HIPCHK(c, hipMemsetAsync(c->d_wq, 0, sizeof(u64) * WQ_WORDS, c->stream));
        const bool partitioned = c->dist_active && c->part_index; /* the lookups travel to the buckets' owners (collective) */
        if (partitioned) CHK(dist_partitioned_probe(c));
        else if (nq) {
            launch_probe(a, range_kernel, grid);
        }
        ph_end(c, DISCO_PH_PROBE_KERNEL);
        HIPCHK(c, hipGetLastError());
        u32 n_big = 0, n_slow = 0;
        if (!partitioned) {
            HIPCHK(c, hipMemcpyAsync(&n_slow, c->d_n_slow, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(&n_big, c->d_n_big, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
        }
        CHK(read_counters(c));
        if (partitioned) c->h_ctr[CTR_HITS_NEEDED] = c->hits_used;
        if (!c->h_ctr[CTR_OVERFLOW] && n_slow) { /* reads without a usable run list, the long way (they may add big rows) */
            int g2 = wave_grid(c, (n_slow + WQ_CHUNK - 1) / WQ_CHUNK, 24);
            HIPCHK(c, hipMemsetAsync(c->d_wq, 0, sizeof(u64) * WQ_WORDS, c->stream));
            launch_probe(a, probe_pick(c, 2, false), g2);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(&n_big, c->d_n_big, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
            CHK(read_counters(c));
        }
        if (!partitioned) c->slow_rows = n_slow;
        if (!c->h_ctr[CTR_OVERFLOW] && n_big) {
            int g2 = wave_grid(c, (n_big + WQ_CHUNK - 1) / WQ_CHUNK, 8);
            HIPCHK(c, hipMemsetAsync(c->d_wq, 0, sizeof(u64) * WQ_WORDS, c->stream));
            launch_probe(a, probe_pick(c, 1, false), g2);
            HIPCHK(c, hipGetLastError());
            CHK(read_counters(c));
        }
        if (!c->h_ctr[CTR_OVERFLOW]) {
            c->big_rows = n_big;
            c->hits_used = c->h_ctr[CTR_HITS_NEEDED];
            VerifyArgs va;
            va.v = view(c);
            va.best = c->d_best;
            va.hits = c->d_hits;
            va.row_start = c->d_row_start;
            va.row_cnt = c->d_row_cnt;
            va.order = c->d_order_used;
            va.meta_ord = c->d_meta_ord;
            if (c->wait_bulk_before_verify) { /* multi-GPU flow: the candidate rows of other ranks' reads arrive on bulk_stream */
                HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_bulk, 0));
                c->wait_bulk_before_verify = false;
            }
            /* two passes (containment-type candidates, flags, overlap-type candidates of non-contained reads) where most reads
             * can be contained: only on request (the kmer_hits counter then counts the compared candidates only), reads of mixed
             * length, rows of the 64-byte staged variants, and not inside a multi-GPU pass (its flags need an exchange in between) */
            /* (multi-GPU pass: every rank takes the same branch — min / max length are the job's, nq plays no part) */
            const bool inexact = c->prm.max_substitutions != 0; /* single pass: the extension is not tuned for metagenomes */
            va.max_subs = c->prm.max_substitutions;
            const bool two_pass = !inexact && !c->two_class && (c->prm.flags & DISCO_FLAG_TWO_PASS_VERIFY) && c->S == VERIFY_SW && (nq || c->dist_active) &&
                                  (u64)c->min_len * 10 < (u64)c->max_len * 9 && !getenv("DISCO_NO_TWO_PASS");
            c->two_pass_last = two_pass;
            /* 64-byte rows, exact overlaps: candidates of a 64-read chunk as one flat list, full wavefronts (verify_flat_kernel) */
            const bool flat = !inexact && c->S == VERIFY_SW && (c->two_class || !getenv("DISCO_NO_FLAT_VERIFY"));
            ph_begin(c, DISCO_PH_VERIFY);
            if (c->two_class && nq) { /* the long reads' candidate rows: out of the flat pass, to verify_long_kernel behind it */
                HIPCHK(c, hipMemsetAsync(c->d_n_list, 0, sizeof(u32), c->stream));
                hipLaunchKernelGGL(class_take_rows_kernel, dim3((unsigned)std::min<u64>((nq + TAKE_SPAN - 1) / TAKE_SPAN, (u64)c->n_cu * 8)), dim3(256), 0, c->stream, c->d_meta_ord,
                                   (const u64 *)c->d_order_used, c->q_lo, nq, (const u32 *)c->d_ovf, c->d_lpos, c->d_lmeta, c->d_linfo, c->d_n_list, (u32)c->n_long);
            }
            if (two_pass) {
                CHK(ensure(c, c->d_contained, c->n_alloc));
                CHK(ensure(c, c->d_cbits, c->n_alloc / 64 + 1));
                va.cbits = c->d_cbits;
                if (nq) verify_launch(c, va, nq, 1, flat, inexact);
                if (c->dist_active) { /* the keys of other ranks' containing reads count too: exchange, then the flags (collective) */
                    CHK(dist_mark_contained(c));
                    c->contained_done = true;
                } else {
                    CHK(zero_counter(c, CTR_N_CONTAINED));
                    hipLaunchKernelGGL(contain_flags_kernel, dim3(flat_grid(c, c->n)), dim3(256), 0, c->stream, c->d_best, c->n, c->d_contained, c->d_cbits, c->d_ctr);
                }
                if (nq) verify_launch(c, va, nq, 2, flat, inexact);
            } else if (nq) {
                va.cbits = nullptr;
                verify_launch(c, va, nq, 0, flat, inexact);
            }
            if (c->two_class && nq)
                wq_launch(c, verify_long_kernel, c->n_long * 16, "DISCO_VL_WAVES", 32, va, (const u32 *)c->d_lpos, (const ulonglong2 *)c->d_lmeta, (const uint2 *)c->d_linfo, (const u32 *)c->d_n_list);
            ph_end(c, DISCO_PH_VERIFY);
            HIPCHK(c, hipGetLastError());
            CHK(read_counters(c));
            ph_collect(c);
            c->es_big_counted = true; /* (h_ctr[CTR_ES_BIG]: rows with more than ES_CAP verified hits) */
            c->phase = 3;
            return DISCO_OK;
        }
        if (getenv("DISCO_VERBOSE"))
            fprintf(stderr, "[disco] probe attempt %d overflowed: hits_cap=%llu needed=%llu n_big=%u big_cap=%u overflow=%llu\n", attempt,
                    (unsigned long long)c->d_hits.cap, (unsigned long long)c->h_ctr[CTR_HITS_NEEDED], n_big, (unsigned)c->d_big_list.cap, (unsigned long long)c->h_ctr[CTR_OVERFLOW]);
        /* something was too small: grow and redo the pass (atomicMin on best is idempotent) */
        if (n_big > c->d_big_list.cap) want_big = (u32)std::min<u64>(nq, (u64)n_big + n_big / 4 + 1024);
        if (n_slow > c->d_slow_list.cap) want_slow = (u32)std::min<u64>(nq, (u64)n_slow + n_slow / 4 + 1024);
        u64 needed = c->h_ctr[CTR_HITS_NEEDED];
        want_hits = std::max<u64>(c->d_hits.cap * 2, needed + needed / 4 + (u64)grid * chunk_slots);
    }
    return fail(c, DISCO_E_CAPACITY, "disco_probe: hit buffer could not be sized");
}


int disco_mark_contained(disco_ctx *c, uint64_t *n_contained)
{
    DISCO_TRACE("disco_mark_contained");
    if (!c) return DISCO_E_ARG;
    if (c->phase < 3) return fail(c, DISCO_E_STATE, "disco_mark_contained: run disco_probe first");
    HIPCHK(c, hipSetDevice(c->device));
    drop_contained_records(c);
    CHK(ensure(c, c->d_contained, c->n_alloc));
    CHK(ensure(c, c->d_cbits, c->n_alloc / 64 + 1));
    CHK(zero_counter(c, CTR_N_CONTAINED));
    ph_begin(c, DISCO_PH_CONTAIN);
    if (c->n) hipLaunchKernelGGL(contain_flags_kernel, dim3(flat_grid(c, c->n)), dim3(256), 0, c->stream, c->d_best, c->n, c->d_contained, c->d_cbits, c->d_ctr);
    HIPCHK(c, hipGetLastError());
    ph_end(c, DISCO_PH_CONTAIN);
    CHK(read_counters(c));
    ph_collect(c);
    c->n_contained = c->h_ctr[CTR_N_CONTAINED];
    if (n_contained) *n_contained = c->n_contained;
    c->phase = 4;
    c->crows_pending = c->cgrp_pending = false; /* rows of other flags */
    return DISCO_OK;
}

/* ---------------------------------------------------------------------------------------------------------------- */
/* the big-item lists (rows / nodes beyond the LDS capacities) must hold every such item: count them first */
static int ensure_big_cap(disco_ctx *c, const u32 *cnt, const u64 *ref, u32 thr)
{
    CHK(zero_counter(c, CTR_ES_BIG));
    /* (ranks own loci: q_lo / q_hi are positions; the rows and reference words of the other ranks' reads are zero) */
    const u64 ilo = c->loci ? 0 : c->q_lo, ihi = c->loci ? c->n : c->q_hi;
    if (ihi > ilo) hipLaunchKernelGGL(count_above_kernel, dim3(flat_grid(c, ihi - ilo)), dim3(256), 0, c->stream, cnt, ref, ilo, ihi, thr, c->d_ctr + CTR_ES_BIG);
    HIPCHK(c, hipGetLastError());
    CHK(read_counters(c));
    const u64 need = c->h_ctr[CTR_ES_BIG] + 1024;
    if (need > 0xFFFFFFFFull) return fail(c, DISCO_E_CAPACITY, "more than 2^32 big rows");
    return grow_big_lists(c, need);
}

static int select_edges(disco_ctx *c)
{
    DISCO_TRACE("select_edges");
    const u64 nq = c->q_hi - c->q_lo;
    CHK(ensure(c, c->d_adj_ref, c->n));
    HIPCHK(c, hipMemsetAsync(c->d_adj_ref, 0, std::max<u64>(c->n, 1) * sizeof(u64), c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_n_big, 0, sizeof(u32), c->stream));
    CHK(zero_counter(c, CTR_CAP_SITES));
    CHK(zero_counter(c, CTR_DROPPED));
    CHK(zero_counter(c, CTR_ES_SLOW));
    CHK(zero_counter(c, CTR_ADJ_TOTAL));
    CHK(zero_counter(c, CTR_OVERFLOW));
    CHK(zero_counter(c, CTR_TR_BIG));
    CHK(zero_counter(c, CTR_TR_MID));
    /* the kernel rewrites rows in place: it cannot be rerun after an overflow, so its big-row list must hold every such row — counted by
     * verify (no pass of its own, no wait in front of the selection), or here */
    /* the variant of edge_select_flat_kernel with five waves per SIMD where at most one row in a hundred has more than 64 verified hits (they
     * go to the big-row list); DISCO_SELECT_SMALL=0 / 1 forces either */
    const bool rows_counted = c->es_big_counted && !getenv("DISCO_COUNT_BIG_ROWS");
    const bool select_small = rows_counted && env_int("DISCO_SELECT_SMALL", c->h_ctr[CTR_ES_MID] * 100 <= nq ? 1 : 0) != 0;
    if (rows_counted) {
        const u64 need = c->h_ctr[select_small ? CTR_ES_MID : CTR_ES_BIG] + 1024;
        if (need > 0xFFFFFFFFull) return fail(c, DISCO_E_CAPACITY, "more than 2^32 big rows");
        CHK(grow_big_lists(c, need));
    } else
        CHK(ensure_big_cap(c, c->d_row_cnt, nullptr, ES_CAP));
    c->es_big_counted = false;
    EdgeSelArgs a;
    a.v = view(c);
    CHK(ensure(c, c->d_dropbits, c->n_alloc / 64 + 1));
    HIPCHK(c, hipMemsetAsync(c->d_dropbits, 0, (c->n_alloc / 64 + 1) * sizeof(u64), c->stream));
    c->drop_lo = c->loci ? 0 : c->q_lo;
    c->drop_hi = c->loci ? 0 : c->q_hi; /* (ranks own loci: the bitmap is complete once the lists have been exchanged: dist_complete_twins) */
    a.dropbits = c->d_dropbits;
    a.hidden_flags = c->prm.max_substitutions != 0;
    a.drop_node = a.drop_key = nullptr;
    a.drop_cap = 0;
    CHK(zero_counter(c, CTR_DROP_ITEMS));
    if (c->prm.max_substitutions == 0 && !getenv("DISCO_NO_DROP_LIST")) {
        CHK(ensure(c, c->d_drop_node, DROP_LIST_CAP));
        CHK(ensure(c, c->d_drop_key, DROP_LIST_CAP));
        a.drop_node = c->d_drop_node;
        a.drop_key = c->d_drop_key;
        a.drop_cap = (u32)std::min<u64>(DROP_LIST_CAP, (u64)env_int("DISCO_DROP_LIST_CAP", (int)DROP_LIST_CAP)); /* (tests: a list that overflows) */
    }
    a.contained = c->d_cbits;
    a.hits = c->d_hits;
    a.row_start = c->d_row_start;
    a.row_cnt = c->d_row_cnt;
    a.ref = c->d_adj_ref;
    a.max_per_kmer = c->prm.max_edges_per_kmer;
    a.big_list = c->d_big_list;
    a.n_big = c->d_n_big;
    a.big_cap = c->d_big_list.cap;
    a.scratch = nullptr;
    a.scratch_cap = 0;
    a.order = c->d_order_used; /* the headers in meta_ord are by position in THIS order */
    a.meta_ord = c->d_meta_ord;
    ph_begin(c, DISCO_PH_SELECT);
    /* reads of up to 256 bases, exact overlaps: the hits of several reads as one flat list, full wavefronts (edge_select_flat_kernel) */
    const bool flat_select = c->S == VERIFY_SW && c->max_len <= 256 && !a.hidden_flags && a.max_per_kmer < 255u && !getenv("DISCO_NO_FLAT_SELECT");
    if (nq) wq_launch(c, edge_select_pick(false, flat_select, select_small), nq, "DISCO_SELECT_WAVES", 32, a);
    ph_end(c, DISCO_PH_SELECT);
    HIPCHK(c, hipGetLastError());
    u32 n_big = 0;
    HIPCHK(c, hipMemcpyAsync(&n_big, c->d_n_big, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    CHK(read_counters(c));
    ph_collect(c);
    if (c->h_ctr[CTR_OVERFLOW]) return fail(c, DISCO_E_CAPACITY, "edge selection: big-row list overflow (%u rows)", n_big);
    if (n_big) { /* rows of up to ES_MID hits: LDS arrays of their own (the five-wave variant lists rows of 65 .. ES_CAP hits too: a pass with small arrays first) */
        if (select_small) {
            HIPCHK(c, hipMemsetAsync(c->d_wq, 0, sizeof(u64) * WQ_WORDS, c->stream));
            hipLaunchKernelGGL(edge_select_mid_kernel<ES_CAP>, dim3((int)std::min<u64>(n_big, (u64)c->n_cu * 32)), dim3(64), 0, c->stream, a, 0u);
        }
        if (!select_small || c->h_ctr[CTR_ES_BIG]) {
            HIPCHK(c, hipMemsetAsync(c->d_wq, 0, sizeof(u64) * WQ_WORDS, c->stream));
            hipLaunchKernelGGL(edge_select_mid_kernel<ES_MID>, dim3((int)std::min<u64>(n_big, (u64)c->n_cu * 8)), dim3(64), 0, c->stream, a, select_small ? (u32)ES_CAP : 0u);
        }
        HIPCHK(c, hipGetLastError());
        CHK(read_counters(c));
    }
    if (n_big && c->h_ctr[CTR_MAX_ROW] > ES_MID) {
        int g2 = (int)std::min<u64>(n_big, (u64)c->n_cu * 8); /* work queue, one big row per grab */
        u64 cap = c->h_ctr[CTR_MAX_ROW] + 64;
        LocalBuf<u64> scratch(c);
        CHK(ensure(c, scratch, (u64)g2 * 2 * cap));
        a.scratch = scratch;
        a.scratch_cap = cap;
        HIPCHK(c, hipMemsetAsync(c->d_wq, 0, sizeof(u64) * WQ_WORDS, c->stream));
        hipLaunchKernelGGL(edge_select_pick(true, false, false), dim3(g2), dim3(64), 0, c->stream, a);
        hipError_t e = hipGetLastError();
        int rc = read_counters(c); /* synchronises before the scratch goes back */
        if (e != hipSuccess) return fail(c, DISCO_E_HIP, "edge_select_kernel (big rows): %s", hipGetErrorString(e));
        CHK(rc);
    }
    c->dropped = c->dropped_local = c->h_ctr[CTR_DROPPED];
    c->n_drop_items = a.drop_node ? c->h_ctr[CTR_DROP_ITEMS] : ~0ull;
    c->tr_big_counted = true; /* (h_ctr[CTR_TR_BIG]: nodes with more than TR_CAP finds) */
    if (c->contained_count_pending) { /* disco_run_graph: the flags' count came back with these counters */
        c->n_contained = c->h_ctr[CTR_N_CONTAINED];
        c->contained_count_pending = false;
    }
    if (getenv("DISCO_VERBOSE"))
        fprintf(stderr, "[disco] edge selection%s: %llu rows in the sequential path, %u in the big-row list (%llu rows of more than 64 hits), dropped %llu\n",
                select_small ? " (five waves per SIMD)" : "", (unsigned long long)c->h_ctr[CTR_ES_SLOW], n_big, (unsigned long long)c->h_ctr[CTR_ES_MID], (unsigned long long)c->dropped);
    /* the finds stay where they are: the hit buffer IS the adjacency array of the local rows */
    c->d_adj = c->d_hits;
    c->adj_total = c->h_ctr[CTR_ADJ_TOTAL];
    c->adj_imported = false;
    c->adj_span = 0;
    c->half_complete = true; /* one rank: the local lists are all the lists */
    c->ph_ms[DISCO_PH_CSR] = 0;
    c->phase = 5;
    return DISCO_OK;
}

/* the few-extras merge moves only the rows that grow; otherwise every row is rebuilt (merge_extras) */
static bool merge_is_sparse(const disco_ctx *c) { return c->d_adj == c->d_hits && c->n_extra <= 16384 && !getenv("DISCO_MERGE_REBUILD"); }

static int twin_check_search(disco_ctx *c, u64 lo, u64 hi);

/* twin check over targets [lo,hi); collects extras, does not merge */
static int twin_check(disco_ctx *c, u64 lo, u64 hi)
{
    CHK(twin_check_search(c, lo, hi));
    /* inexact overlaps: edge selection left "hidden from the other read" flags in the entries (ADJ_HIDDEN_OF); rows that the merge
     * does not rebuild are cleaned here */
    if (c->prm.max_substitutions != 0 && c->n && (c->n_extra == 0 || merge_is_sparse(c))) {
        hipLaunchKernelGGL(clear_adj_flags_kernel, dim3(flat_grid(c, c->n * 16)), dim3(256), 0, c->stream, c->d_adj_ref, c->d_adj, c->n);
        HIPCHK(c, hipGetLastError());
    }
    return DISCO_OK;
}

static int twin_check_search(disco_ctx *c, u64 lo, u64 hi)
{
    DISCO_TRACE("twin_check");
    CHK(ensure(c, c->d_extra_cnt, c->n));
    /* After the contained filter the verified-hit relation is symmetric: a hit A->B at window j >= 1 of overlap length
     * ovl >= k+1 shows up from B's side at window ovl-k >= 1 against A's other end record, and verifies over the same
     * region. A find can therefore miss its twin only if the twin's owner DROPPED a verified hit (second hit to the same
     * destination, BG/OverlapGraph.cpp:656, or the per-k-mer cap, :645). If no read of the target range dropped anything,
     * every list in the range already holds all twins and nothing needs to be searched. */
    /* (inexact mode: a substitution inside one read's end k-mer hides the pair from the other side — always search) */
    if (c->dropped == 0 && c->prm.max_substitutions == 0 && lo >= c->q_lo && hi <= c->q_hi && !getenv("DISCO_FORCE_TWIN_CHECK")) {
        c->n_extra = 0;
        c->asym_local = 0;
        c->ph_ms[DISCO_PH_TWIN] = 0;
        return DISCO_OK;
    }
    TwinArgs a;
    a.v = view(c);
    a.ref = c->d_adj_ref;
    a.adj = c->d_adj;
    a.lo = lo;
    a.hi = hi;
    a.otab = c->loci ? c->d_otab : nullptr; /* (ranks own loci: of the nodes [lo, hi) only the own ones) */
    a.me = c->comm ? (u32)c->comm->rank : 0u;
    a.extra_cnt = c->d_extra_cnt;
    a.n_extra = c->d_n_extra;
    /* Something was dropped — but only the lists of the reads that dropped something can lack a twin (same argument, per read):
     * with their bitmap at hand the search is limited to finds INTO those reads, a few thousand instead of every entry of
     * every list (real data always drop something at their repeats: 95 -> 5 ms at 50 M reads with 0.3 % errors) */
    /* One GPU, exact overlaps: the dropped hits themselves are on a list (every one of them, or the list is not used). A twin is missing
     * from w's list only where w dropped exactly that hit, so each item is looked up once in the OTHER read's list — no pass over the
     * entries at all (16 -> 0.1 ms at 50 M reads with 0.1 % errors) */
    const bool by_list = c->prm.max_substitutions == 0 && c->d_drop_node && lo == 0 && hi == c->n && c->q_lo == 0 && c->q_hi == c->n && !c->adj_imported &&
                         c->n_drop_items == c->dropped && c->n_drop_items <= (u64)env_int("DISCO_DROP_LIST_CAP", (int)DROP_LIST_CAP) && !getenv("DISCO_FORCE_TWIN_CHECK");
    const bool by_bitmap = !by_list && c->d_dropbits && lo >= c->drop_lo && hi <= c->drop_hi && !getenv("DISCO_FORCE_TWIN_CHECK");
    a.dropbits = by_bitmap ? c->d_dropbits : nullptr;
    /* inexact overlaps: the same, plus every find verify_kernel flagged as hidden from the other read (a substitution inside this
     * read's end k-mer there) — 0.13 -> 0.04 s of search at 50 M reads with 0.3 % errors */
    a.hidden_flags = by_bitmap && c->prm.max_substitutions != 0;
    /* (inexact overlaps: one-sided pairs are the rule — a substitution inside an end k-mer hides the pair from the other read —
     * so the proof of symmetry is not attempted) */
    if (!by_bitmap && !by_list && c->prm.max_substitutions == 0) {   /* one-sided pass: half the searches, no extras. Symmetric iff nothing is missing and #up == #down. */
        CHK(zero_counter(c, CTR_ASYM));
        CHK(zero_counter(c, CTR_TW_UP));
        CHK(zero_counter(c, CTR_TW_DOWN));
        a.extra_node = nullptr;
        a.extra_key = nullptr;
        a.extra_cap = 0;
        a.up_only = 1;
        ph_begin(c, DISCO_PH_TWIN);
        if (c->n) hipLaunchKernelGGL(twin_check_kernel, dim3(flat_grid(c, c->n * 64)), dim3(256), 0, c->stream, a);
        ph_end(c, DISCO_PH_TWIN);
        HIPCHK(c, hipGetLastError());
        CHK(read_counters(c));
        ph_collect(c);
        if (getenv("DISCO_VERBOSE"))
            fprintf(stderr, "[disco] twin check [%llu,%llu): one-sided pass: missing %llu, up %llu, down %llu (dropped %llu)\n", (unsigned long long)lo,
                    (unsigned long long)hi, (unsigned long long)c->h_ctr[CTR_ASYM], (unsigned long long)c->h_ctr[CTR_TW_UP],
                    (unsigned long long)c->h_ctr[CTR_TW_DOWN], (unsigned long long)c->dropped);
        if (c->h_ctr[CTR_ASYM] == 0 && c->h_ctr[CTR_TW_UP] == c->h_ctr[CTR_TW_DOWN]) {
            c->n_extra = 0;
            c->asym_local = 0;
            return DISCO_OK;
        }
    }
    u32 want = std::max<u32>(4096, extra_cap(c)); /* the lists kept from the last pass are the best guess */
    if (by_list) want = std::max<u32>(want, (u32)c->n_drop_items); /* (an item yields at most one extra) */
    for (int attempt = 0; attempt < 6; attempt++) {
        CHK(ensure_group(c, want, want, c->d_extra_node, c->d_extra_key));
        HIPCHK(c, hipMemsetAsync(c->d_extra_cnt, 0, std::max<u64>(c->n, 1) * sizeof(u32), c->stream));
        HIPCHK(c, hipMemsetAsync(c->d_n_extra, 0, sizeof(u32), c->stream));
        CHK(zero_counter(c, CTR_ASYM));
        CHK(zero_counter(c, CTR_OVERFLOW));
        a.extra_node = c->d_extra_node;
        a.extra_key = c->d_extra_key;
        a.extra_cap = extra_cap(c);
        a.up_only = 0;
        ph_begin(c, DISCO_PH_TWIN);
        if (by_list) {
            if (c->n_drop_items)
                hipLaunchKernelGGL(twin_from_drops_kernel, dim3(flat_grid(c, c->n_drop_items)), dim3(256), 0, c->stream, a, (const u64 *)c->d_drop_node,
                                   (const u64 *)c->d_drop_key, (u32)c->n_drop_items);
        } else if (c->n)
            hipLaunchKernelGGL(twin_check_kernel, dim3(flat_grid(c, c->n * 64)), dim3(256), 0, c->stream, a);
        ph_end(c, DISCO_PH_TWIN);
        HIPCHK(c, hipGetLastError());
        u32 ne = 0;
        HIPCHK(c, hipMemcpyAsync(&ne, c->d_n_extra, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
        CHK(read_counters(c));
        ph_collect(c);
        if (!c->h_ctr[CTR_OVERFLOW]) {
            c->n_extra = ne;
            c->asym_local = c->h_ctr[CTR_ASYM];
            /* a partial range: the one-sided pass was unbalanced, i.e. a down-find FROM this range has no twin — but that twin is
             * missing from the list of a node of ANOTHER range, which this pass does not complete. Report "not symmetric" all the
             * same: the sharded caller sums these values over the ranks only to decide whether every rank must run the full pass
             * (found by tools/fuzz_sharded.py: one cap-bound site on rank 0, both ranks answered 0) */
            if (c->asym_local == 0 && !(lo == 0 && hi == c->n)) c->asym_local = 1;
            return DISCO_OK;
        }
        want = ne + ne / 4 + 4096;
    }
    return fail(c, DISCO_E_CAPACITY, "twin check: extras list could not be sized");
}

/* merge the collected extras into a node-ordered CSR (rare: only when pairs were found from one side only) */
static int merge_extras(disco_ctx *c)
{
    DISCO_TRACE("merge_extras");
    if (c->n_extra == 0) return DISCO_OK;
    c->tr_big_counted = false; /* rows grow */
    /* a handful of extras and the rows still where edge selection left them (one GPU): move only the rows that grow into the free
     * tail of the hit buffer — 84 ms of the 272 ms pass at 50 M reads with 0.3 % errors went into rebuilding all of it for 953 extras */
    if (merge_is_sparse(c)) {
        HIPCHK(c, hipMemsetAsync(c->d_bump, 0, sizeof(u64), c->stream));
        hipLaunchKernelGGL(merge_need_kernel, dim3(flat_grid(c, c->n)), dim3(256), 0, c->stream, c->d_adj_ref, c->d_extra_cnt, c->n, c->d_bump);
        u64 need = 0;
        HIPCHK(c, hipMemcpyAsync(&need, c->d_bump, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->hits_used + need <= c->d_hits.cap) {
            HIPCHK(c, hipMemsetAsync(c->d_bump, 0, sizeof(u64), c->stream));
            hipLaunchKernelGGL(merge_sparse_kernel, dim3((unsigned)std::min<u64>(c->n_extra, (u64)c->n_cu * 16)), dim3(64), 0, c->stream, c->d_extra_node, c->d_extra_key,
                               c->n_extra, c->d_extra_cnt, c->d_adj_ref, c->d_adj, c->hits_used, c->d_bump);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipStreamSynchronize(c->stream));
            c->hits_used += need;
            c->adj_total += c->n_extra;
            c->n_extra = 0;
            return DISCO_OK;
        }
    }
    LocalBuf<u32> new_deg(c);
    LocalBuf<u64> new_start(c), new_adj(c), scratch(c);
    u64 total = 0;
    CHK(ensure(c, new_deg, c->n));
    CHK(ensure(c, new_start, c->n + 1));
    hipLaunchKernelGGL(merge_deg_kernel, dim3(flat_grid(c, c->n)), dim3(256), 0, c->stream, c->d_adj_ref, c->d_extra_cnt, c->n, new_deg);
    CHK((scan_exclusive<u32, u64>(c, new_deg, c->n, new_start, true, &total)));
    if (c->d_adj_spare.cap >= total && c->d_adj_spare) /* the buffer the previous pass's merge left behind */
        new_adj.take(c->d_adj_spare);
    else
        CHK(ensure(c, new_adj, total + total / 16));
    hipLaunchKernelGGL(merge_scatter_kernel, dim3(flat_grid(c, c->n_extra)), dim3(256), 0, c->stream, c->d_extra_node, c->d_extra_key, c->n_extra, c->d_adj_ref, new_start, new_adj);
    /* row scratch: the longest merged row (reduced on the device) */
    CHK(zero_counter(c, CTR_MAX_DEG));
    hipLaunchKernelGGL(max_u32_kernel, dim3(flat_grid(c, c->n)), dim3(256), 0, c->stream, new_deg, c->n, c->d_ctr + CTR_MAX_DEG);
    HIPCHK(c, hipGetLastError());
    CHK(read_counters(c));
    const u64 maxdeg = c->h_ctr[CTR_MAX_DEG];
    const int g = (int)std::min<u64>(c->n, (u64)c->n_cu * 32); /* one wavefront per row at a time */
    CHK(ensure(c, scratch, (u64)g * (maxdeg + 1)));
    hipLaunchKernelGGL(merge_rows_kernel, dim3(g), dim3(64), 0, c->stream, c->d_adj_ref, c->d_adj, c->d_extra_cnt, new_start, new_adj, c->n, scratch, maxdeg + 1);
    hipLaunchKernelGGL(ref_from_start_kernel, dim3(flat_grid(c, c->n)), dim3(256), 0, c->stream, new_start, new_deg, c->n, c->d_adj_ref);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    /* the rows move to new_adj; what held the imported / merged rows so far waits for the next pass's merge */
    release(c, c->d_adj_spare);
    c->d_adj_spare = c->d_adj_own;
    c->d_adj_own = DevBuf<u64>();
    new_adj.give(c->d_adj_own);
    c->d_adj = c->d_adj_own;
    c->adj_total = total;
    c->adj_span = total; /* compact, node ordered */
    c->n_extra = 0;
    return DISCO_OK;
}

int disco_select_edges(disco_ctx *c)
{
    if (!c) return DISCO_E_ARG;
    if (c->phase != 4) return fail(c, DISCO_E_STATE, "disco_select_edges: run disco_mark_contained first");
    HIPCHK(c, hipSetDevice(c->device));
    return select_edges(c);
}

/* full != 0: check (and complete) the lists of ALL nodes; else only those of the query range */
int disco_symmetrize(disco_ctx *c, int full, uint64_t *n_asym)
{
    if (!c) return DISCO_E_ARG;
    if (c->phase < 5) return fail(c, DISCO_E_STATE, "disco_symmetrize: select edges first");
    HIPCHK(c, hipSetDevice(c->device));
    CHK(twin_check(c, full ? 0 : c->q_lo, full ? c->n : c->q_hi));
    if (n_asym) *n_asym = c->asym_local;
    c->phase = 6;
    return DISCO_OK;
}

int disco_merge_extras(disco_ctx *c)
{
    if (!c) return DISCO_E_ARG;
    if (c->phase < 6) return fail(c, DISCO_E_STATE, "disco_merge_extras: symmetrize first");
    HIPCHK(c, hipSetDevice(c->device));
    return merge_extras(c);
}

int disco_build_edges(disco_ctx *c, uint64_t *n_pre)
{
    if (!c) return DISCO_E_ARG;
    CHK(disco_select_edges(c));
    CHK(disco_symmetrize(c, 1, nullptr));
    CHK(merge_extras(c));
    if (n_pre) *n_pre = c->adj_total / 2;
    return DISCO_OK;
}

int disco_adjacency_size(disco_ctx *c, uint64_t *n_entries)
{
    if (!c || !n_entries) return DISCO_E_ARG;
    if (c->phase < 5) return fail(c, DISCO_E_STATE, "disco_adjacency_size: select edges first");
    *n_entries = c->adj_total;
    return DISCO_OK;
}

int disco_export_adjacency(disco_ctx *c, void *d_deg_u32, void *d_entries_u64)
{
    if (!c || !d_deg_u32) return DISCO_E_ARG;
    if (c->phase < 5 || c->adj_imported) return fail(c, DISCO_E_STATE, "disco_export_adjacency: needs the locally selected edges");
    HIPCHK(c, hipSetDevice(c->device));
    const u64 nq = c->q_hi - c->q_lo;
    ph_begin(c, DISCO_PH_CSR);
    if (nq) hipLaunchKernelGGL(deg_from_ref_kernel, dim3(flat_grid(c, nq)), dim3(256), 0, c->stream, c->d_adj_ref, c->q_lo, c->q_hi, (u32 *)d_deg_u32);
    HIPCHK(c, hipGetLastError());
    if (nq && c->adj_total && d_entries_u64) { /* compact the local rows into node order */
        CHK(ensure(c, c->d_start_tmp, c->n + 1));
        u64 *start = c->d_start_tmp;
        u64 total = 0;
        int rc = scan_exclusive<u32, u64>(c, (const u32 *)d_deg_u32, nq, start, true, &total);
        if (rc == DISCO_OK && total != c->adj_total) rc = fail(c, DISCO_E_STATE, "disco_export_adjacency: degree sum %llu != %llu", (unsigned long long)total, (unsigned long long)c->adj_total);
        if (rc == DISCO_OK) hipLaunchKernelGGL(rows_gather_kernel, dim3(wave_grid(c, nq, 16)), dim3(64), 0, c->stream, c->d_adj, c->d_adj_ref, c->q_lo, c->q_hi, start, (u64 *)d_entries_u64,
                                              (c->phase == 5 && c->prm.max_substitutions != 0) ? 0ull : (u64)ADJ_FLAG); /* (hidden flags travel to the twin search) */
        hipError_t e = hipStreamSynchronize(c->stream);
        CHK(rc);
        if (e != hipSuccess) return fail(c, DISCO_E_HIP, "disco_export_adjacency: %s", hipGetErrorString(e));
    }
    ph_end(c, DISCO_PH_CSR);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    ph_collect(c);
    return DISCO_OK;
}





int disco_import_adjacency(disco_ctx *c, const void *d_deg_u32_all, const void *d_entries_u64_all, uint64_t n_entries_all)
{
    if (!c || !d_deg_u32_all) return DISCO_E_ARG;
    if (c->phase < 5) return fail(c, DISCO_E_STATE, "disco_import_adjacency: select edges first");
    HIPCHK(c, hipSetDevice(c->device));
    CHK(ensure(c, c->d_start_tmp, c->n + 1));
    u64 *start = c->d_start_tmp;
    u64 total = 0;
    CHK((scan_exclusive<u32, u64>(c, (const u32 *)d_deg_u32_all, c->n, start, true, &total)));
    if (total != n_entries_all)
        return fail(c, DISCO_E_ARG, "disco_import_adjacency: degrees sum to %llu but %llu entries were passed", (unsigned long long)total, (unsigned long long)n_entries_all);
    CHK(ensure(c, c->d_adj_own, total));
    c->d_adj = c->d_adj_own;
    c->adj_total = total;
    if (total) HIPCHK(c, hipMemcpyAsync(c->d_adj, d_entries_u64_all, total * 8, hipMemcpyDeviceToDevice, c->stream));
    if (c->n) hipLaunchKernelGGL(ref_from_start_kernel, dim3(flat_grid(c, c->n)), dim3(256), 0, c->stream, start, (const u32 *)d_deg_u32_all, c->n, c->d_adj_ref);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->adj_imported = true;
    c->tr_big_counted = false;
    c->adj_span = total;
    c->half_complete = false;
    c->phase = 5;
    return DISCO_OK;
}




/* ---------------------------------------------------------------------------------------------------------------- */
int disco_transitive_mark(disco_ctx *c)
{
    DISCO_TRACE("disco_transitive_mark");
    if (!c) return DISCO_E_ARG;
    if (c->phase < 6) return fail(c, DISCO_E_STATE, "disco_transitive_mark: build edges first");
    HIPCHK(c, hipSetDevice(c->device));
    const u64 nq = c->q_hi - c->q_lo;
    HIPCHK(c, hipMemsetAsync(c->d_n_big, 0, sizeof(u32), c->stream));
    CHK(zero_counter(c, CTR_OVERFLOW));
    /* the variant with LDS arrays for TR_CAP_SMALL neighbours (eight waves per SIMD) where at most one node in a hundred is beyond them
     * (they go to the big-node pass); DISCO_TR_SMALL=0 / 1 forces either */
    const bool counted_nodes = c->tr_big_counted && c->q_lo == 0 && c->q_hi == c->n && !getenv("DISCO_COUNT_BIG_ROWS");
    const bool tr_small = env_int("DISCO_TR_SMALL", counted_nodes && c->h_ctr[CTR_TR_MID] * 100 <= nq ? 1 : 0) != 0 && counted_nodes;
    if (counted_nodes) { /* edge selection counted the nodes beyond TR_CAP (and beyond TR_CAP_SMALL) */
        const u64 need = c->h_ctr[tr_small ? CTR_TR_MID : CTR_TR_BIG] + 1024;
        if (need > 0xFFFFFFFFull) return fail(c, DISCO_E_CAPACITY, "more than 2^32 big nodes");
        CHK(grow_big_lists(c, need));
    } else
        CHK(ensure_big_cap(c, nullptr, c->d_adj_ref, TR_CAP));
    c->use_half = !getenv("DISCO_NO_HALF");
    /* every row needs its flags when the emission cannot rely on the survivor lists alone */
    const u32 all_flags = (c->adj_imported || !c->use_half || c->q_lo != 0 || c->q_hi != c->n) ? 1u : 0u;
    const bool lists = c->use_half && !all_flags; /* the survivor lists are the result: self-delimiting, and the variant compiled for it */
    TrArgs a;
    CHK(tr_args_begin(c, &a, lists));
    a.order = (c->d_order_used && c->order_q_lo == c->q_lo && c->order_q_hi == c->q_hi && !c->adj_imported && !getenv("DISCO_TR_NO_ORDER")) ? c->d_order_used : nullptr;
    a.all_flags = all_flags;
    ph_begin(c, DISCO_PH_TRMARK);
    if (nq) wq_launch(c, tr_pick(false, false, tr_small, lists), nq, "DISCO_TR_WAVES", 32, a);
    ph_end(c, DISCO_PH_TRMARK);
    HIPCHK(c, hipGetLastError());
    u32 n_big = 0;
    HIPCHK(c, hipMemcpyAsync(&n_big, c->d_n_big, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    c->n_wide = 0;
    if (c->use_half) HIPCHK(c, hipMemcpyAsync(&c->n_wide, c->d_n_wide, sizeof(u32), hipMemcpyDeviceToHost, c->stream)); /* (read again below if the big nodes add to it) */
    CHK(read_counters(c));
    ph_collect(c);
    if (c->h_ctr[CTR_OVERFLOW]) return fail(c, DISCO_E_CAPACITY, "transitive marking: big-node list overflow (%u nodes)", n_big);
    if (n_big) {
        CHK(tr_big_nodes(c, &a, n_big, false, "big nodes"));
        if (c->h_ctr[CTR_OVERFLOW]) return fail(c, DISCO_E_CAPACITY, "transitive marking (big nodes): list overflow");
    }
    if (n_big && c->use_half) HIPCHK(c, hipMemcpy(&c->n_wide, c->d_n_wide, sizeof(u32), hipMemcpyDeviceToHost));
    c->flags_pending = false;
    c->phase = 7;
    return DISCO_OK;
}


int disco_emit_edges(disco_ctx *c, uint64_t *n_out)
{
    DISCO_TRACE("disco_emit_edges");
    if (!c) return DISCO_E_ARG;
    if (c->phase < 7) return fail(c, DISCO_E_STATE, "disco_emit_edges: run disco_transitive_mark first");
    HIPCHK(c, hipSetDevice(c->device));
    drop_edge_records(c);
    const u64 nq = c->q_hi - c->q_lo;
    ph_begin(c, DISCO_PH_EMIT);
    const int grid = wq_grid(c, emit_kernel<false>, nq, "DISCO_EMIT_WAVES"); /* (the dense instantiation over the few wide nodes takes it too: 4 KB of LDS more) */
    const u64 n_push = c->dist_active ? c->n_push_r : 0; /* multi-GPU flow: survivors pushed by the owners of the larger endpoints */
    const int grid_push = (int)std::max<u64>(std::min<u64>((n_push + 63) / 64, (u64)c->n_cu * 16), 1);
    const u64 nwaves = (u64)grid * 2 + (n_push ? (u64)grid_push : 0); /* emit_half_kernel + emit_kernel (+ emit_push_recv_kernel) */
    u64 want = std::max<u64>(2 * nq, 1024) + n_push + nwaves * EMIT_CHUNK;
    for (int attempt = 0; attempt < 6; attempt++) {
        CHK(ensure_group(c, want, want, c->d_out_src, c->d_out_ent));
        HIPCHK(c, hipMemsetAsync(c->d_bump, 0, sizeof(u64), c->stream));
        const bool half_emit = c->use_half && c->half_complete; /* else: rows + flags of every node (sharded fallback) */
        /* self-delimiting lists (the whole-table pass of one GPU): both emitters append exact counts — no tails, nothing to compact */
        const bool dense = half_emit && c->half_selfdel && !c->dist_active;
        if (half_emit && c->half_selfdel && !dense) return fail(c, DISCO_E_STATE, "disco_emit_edges: self-delimiting lists under a communicator");
        c->out_dense = dense;
        if (half_emit && nq) {
            EmitHalfArgs h;
            h.v = view(c);
            h.ref = c->d_adj_ref;
            h.adj = c->d_adj;
            h.half = c->d_half;
            h.hcnt = dense ? nullptr : (const u32 *)c->d_hcnt;
            h.out_src = c->d_out_src;
            h.out_ent = c->d_out_ent;
            h.out_cap = c->d_out_src.cap;
            h.bump = c->d_bump;
            h.local_only = c->dist_active ? 1u : 0u;
            h.own = own_set(c);
            h.order = nullptr; /* (tried for one GPU, round 5: the nodes in processing order — 5.3 instead of 3.4 ms: the node's own entries become the random fetches) */
            if (dense) {
                const int gh = wq_grid(c, emit_half_lists_kernel, (nq + 63) / 64, "DISCO_EMIT_WAVES");
                hipLaunchKernelGGL(emit_half_lists_kernel, dim3(gh), dim3(64), 0, c->stream, h);
            } else {
                const int gh = wq_grid(c, emit_half_kernel, (nq + 63) / 64, "DISCO_EMIT_WAVES");
                hipLaunchKernelGGL(emit_half_kernel, dim3(gh), dim3(64), 0, c->stream, h);
            }
        }
        EmitArgs a;
        a.v = view(c);
        a.ref = c->d_adj_ref;
        a.adj = c->d_adj;
        a.hcnt = half_emit && !dense ? (const u32 *)c->d_hcnt : nullptr;
        a.half = half_emit ? c->d_half : nullptr;
        const bool listed = half_emit && c->n_wide <= c->d_wide.cap; /* else the list overflowed: scan the whole range */
        a.list = listed ? c->d_wide : nullptr;
        a.n_list = listed ? c->n_wide : 0;
        a.out_src = c->d_out_src;
        a.out_ent = c->d_out_ent;
        a.out_cap = c->d_out_src.cap;
        a.bump = c->d_bump;
        a.local_only = c->dist_active ? 1u : 0u;
        a.own = own_set(c);
        HIPCHK(c, hipMemsetAsync(c->d_wq, 0, sizeof(u64) * WQ_WORDS, c->stream));
        if (nq && !(listed && c->n_wide == 0)) {
            if (dense) hipLaunchKernelGGL(emit_kernel<true>, dim3(grid), dim3(64), 0, c->stream, a);
            else hipLaunchKernelGGL(emit_kernel<false>, dim3(grid), dim3(64), 0, c->stream, a);
        }
        if (n_push) {
            EmitRecvArgs pr;
            pr.items = c->d_push_r;
            pr.n_items = n_push;
            pr.ref = c->d_adj_ref;
            pr.adj = c->d_adj;
            pr.half = c->d_half;
            pr.hcnt = c->d_hcnt;
            pr.out_src = c->d_out_src;
            pr.out_ent = c->d_out_ent;
            pr.out_cap = c->d_out_src.cap;
            pr.bump = c->d_bump;
            pr.wq = c->d_wq;
            HIPCHK(c, hipMemsetAsync(c->d_wq, 0, sizeof(u64) * WQ_WORDS, c->stream));
            hipLaunchKernelGGL(emit_push_recv_kernel, dim3(grid_push), dim3(64), 0, c->stream, pr);
        }
        HIPCHK(c, hipGetLastError());
        u64 used = 0;
        HIPCHK(c, hipMemcpyAsync(&used, c->d_bump, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (used <= c->d_out_src.cap) {
            c->out_used = used;
            break;
        }
        want = used + used / 8 + nwaves * EMIT_CHUNK;
        if (attempt == 5) return fail(c, DISCO_E_CAPACITY, "disco_emit_edges: output buffer could not be sized");
    }
    /* survivors = chunk slots that are not the ~0 tail marker: count them (the compaction happens at fetch time) */
    u64 total = 0;
    if (c->out_dense) { /* the bump pointer is the number of edges; the consumers take null valid / pos as "slot i is edge i" */
        total = c->out_used;
        release(c, c->d_out_valid);
        release(c, c->d_out_pos);
    } else if (c->out_used) {
        if (c->out_used > c->d_out_valid.cap || c->out_used + 1 > c->d_out_pos.cap) { /* (grown together; sized by the output buffer) */
            release(c, c->d_out_valid);
            release(c, c->d_out_pos);
            int rc = ensure(c, c->d_out_valid, c->d_out_src.cap);
            if (rc == DISCO_OK) rc = ensure(c, c->d_out_pos, c->d_out_src.cap + 1);
            if (rc != DISCO_OK) {
                release(c, c->d_out_valid);
                return rc;
            }
        }
        hipLaunchKernelGGL(emit_valid_kernel, dim3(flat_grid(c, c->out_used)), dim3(256), 0, c->stream, c->d_out_src, c->out_used, c->d_out_valid);
        CHK((scan_exclusive<u8, u64>(c, c->d_out_valid, c->out_used, c->d_out_pos, true, nullptr)));
        HIPCHK(c, hipMemcpyAsync(&total, c->d_total, sizeof(u64), hipMemcpyDeviceToHost, c->stream)); /* (with the phase's one wait) */
    }
    ph_end(c, DISCO_PH_EMIT);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    ph_collect(c);
    c->n_out = total;
    if (n_out) *n_out = total;
    c->phase = 8;
    return DISCO_OK;
}

int disco_transitive_reduce(disco_ctx *c, uint64_t *n_out)
{
    CHK(disco_transitive_mark(c));
    return disco_emit_edges(c, n_out);
}

int disco_run_graph(disco_ctx *c)
{
    DISCO_TRACE("disco_run_graph");
    const bool verbose = getenv("DISCO_VERBOSE") != nullptr;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    auto t0 = now();
    CHK(disco_build_index(c));
    auto t1 = now();
    CHK(disco_probe(c));
    auto t2 = now();
    { /* disco_mark_contained without its wait: the count of the flags comes back with edge selection's counters */
        CHK(ensure(c, c->d_contained, c->n_alloc));
        CHK(ensure(c, c->d_cbits, c->n_alloc / 64 + 1));
        CHK(zero_counter(c, CTR_N_CONTAINED));
        ph_begin(c, DISCO_PH_CONTAIN);
        if (c->n) hipLaunchKernelGGL(contain_flags_kernel, dim3(flat_grid(c, c->n)), dim3(256), 0, c->stream, c->d_best, c->n, c->d_contained, c->d_cbits, c->d_ctr);
        HIPCHK(c, hipGetLastError());
        ph_end(c, DISCO_PH_CONTAIN);
        c->contained_count_pending = true;
        c->phase = 4;
        c->crows_pending = c->cgrp_pending = false;
    }
    auto t3 = now();
    CHK(disco_build_edges(c, nullptr));
    auto t4 = now();
    int rc = disco_transitive_reduce(c, nullptr);
    auto t5 = now();
    if (verbose)
        fprintf(stderr, "[disco] host wall ms: index %.1f probe %.1f contain %.1f edges %.1f reduce %.1f\n", ms(t0, t1), ms(t1, t2), ms(t2, t3), ms(t3, t4), ms(t4, t5));
    return rc;
}

/* ---------------------------------------------------------------------------------------------------------------- */
static int ensure_host_len(disco_ctx *c)
{
    std::lock_guard<std::mutex> lk(c->h_len_mu);
    if (c->h_len_ok && c->h_len.size() == c->n) return DISCO_OK;
    c->h_len.resize(c->n);
    if (c->n) HIPCHK(c, hipMemcpy(c->h_len.data(), c->d_len, c->n * 2, hipMemcpyDeviceToHost));
    c->h_len_ok = true;
    return DISCO_OK;
}

int64_t disco_fetch_contained(disco_ctx *c, disco_contained_row *out, uint64_t cap)
{
    DISCO_TRACE("disco_fetch_contained");
    if (!c) return DISCO_E_ARG;
    if (c->phase < 4) return fail(c, DISCO_E_STATE, "disco_fetch_contained: run disco_mark_contained first");
    HIPCHK(c, hipSetDevice(c->device));
    const u64 nc = c->n_contained;
    if (!out) return (int64_t)nc;
    if (cap < nc) return fail(c, DISCO_E_ARG, "disco_fetch_contained: need room for %llu rows", (unsigned long long)nc);
    if (nc == 0) return 0;
    /* lens_h: len2 | len1 << 16 per row where the device sent them along; null: gathered from the host's copy of the length table */
    auto decode = [&](auto id_of, const u64 *keys_h, const u32 *lens_h) {
        const u16 *hlen = lens_h ? nullptr : c->h_len.data();
        const u32 kk = (u32)c->k;
        parallel_for(nc, [&, hlen, kk, lens_h](u64 b, u64 e_) {
            for (u64 i = b; i < e_; i++) {
                const u64 key = keys_h[i];
                disco_contained_row &r = out[i];
                r.contained = id_of(i);
                r.super = CKEY_SUPER(key);
                r.j = CKEY_J(key);
                r.type = disco_hit_type(CKEY_SUFFIX(key), CKEY_REV(key));
                r.len2 = lens_h ? (lens_h[i] & 0xFFFFu) : hlen[r.contained];
                r.len1 = lens_h ? (lens_h[i] >> 16) : hlen[r.super];
                u32 orient, off;
                disco_map_type(r.type, r.len1, kk, r.j, &orient, &off); /* BG/OverlapGraph.cpp:428-434 */
                r.orient = orient;
                r.start = off;
            }
        });
    };
    CHK(start_contained_rows(c, false));
    if (c->crows_pending && c->crows_n == nc) {
        HIPCHK(c, hipEventSynchronize(c->ev_crows));
        const u64 *hkey = (const u64 *)c->h_crows;
        const u32 *hid = (const u32 *)(hkey + c->crows_hcap);
        decode([hid](u64 i) { return (u64)hid[i]; }, hkey, hid + c->crows_hcap);
        return (int64_t)nc;
    }
    CHK(ensure_host_len(c));
    CHK(settle_keys(c));
    LocalBuf<u64> pos(c), ids(c), keys(c);
    std::vector<u64> hid(nc), hkey(nc);
    CHK(ensure(c, pos, c->n + 1));
    CHK(ensure(c, ids, nc));
    CHK(ensure(c, keys, nc));
    CHK((scan_exclusive<u8, u64>(c, c->d_contained, c->n, pos, false, nullptr)));
    hipLaunchKernelGGL(contain_rows_kernel, dim3(flat_grid(c, c->n)), dim3(256), 0, c->stream, c->d_best, c->d_contained, pos, c->n, ids, keys);
    HIPCHK(c, hipMemcpyAsync(hid.data(), ids, nc * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(hkey.data(), keys, nc * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (u64 i = 0; i < nc; i++) /* (a key that names no read must not index the length table: fail loudly) */
        if (CKEY_SUPER(hkey[i]) >= c->n || hid[i] >= c->n)
            return fail(c, DISCO_E_STATE, "disco_fetch_contained: row %llu of %llu: read %llu has the key %llx (no containing read)", (unsigned long long)i, (unsigned long long)nc,
                        (unsigned long long)hid[i], (unsigned long long)hkey[i]);
    decode([&hid](u64 i) { return hid[i]; }, hkey.data(), nullptr);
    return (int64_t)nc;
}

int64_t disco_fetch_contained_grouped(disco_ctx *c, disco_contained_row *out, uint64_t cap)
{
    DISCO_TRACE("disco_fetch_contained_grouped");
    if (!c) return DISCO_E_ARG;
    if (c->phase < 4) return fail(c, DISCO_E_STATE, "disco_fetch_contained_grouped: run disco_mark_contained first");
    HIPCHK(c, hipSetDevice(c->device));
    const u64 nc = c->n_contained;
    if (!out) return (int64_t)nc;
    if (cap < nc) return fail(c, DISCO_E_ARG, "disco_fetch_contained_grouped: need room for %llu rows", (unsigned long long)nc);
    if (nc == 0) return 0;
    if (getenv("DISCO_NO_GROUPED_ROWS")) return fail(c, DISCO_E_UNSUPPORTED, "disco_fetch_contained_grouped: switched off (DISCO_NO_GROUPED_ROWS)");
    CHK(start_contained_rows(c, true));
    if (!(c->cgrp_pending && c->crows_pending && c->crows_n == nc))
        return fail(c, DISCO_E_UNSUPPORTED, "disco_fetch_contained_grouped: the rows were not grouped on the device (sort what disco_fetch_contained returns)");
    HIPCHK(c, hipStreamSynchronize(c->aux_stream));
    if (c->h_cgrp_big) return fail(c, DISCO_E_UNSUPPORTED, "disco_fetch_contained_grouped: a containing read has more than %d rows (sort what disco_fetch_contained returns)", CROW_GROUP_MAX);
    const u64 *hkey = (const u64 *)((const char *)c->h_crows + c->crows_hcap * 16);
    const u32 *hid = (const u32 *)(hkey + c->crows_hcap), *hln = hid + c->crows_hcap;
    const u32 kk = (u32)c->k;
    parallel_for(nc, [&, kk, hkey, hid, hln](u64 b, u64 e_) {
        for (u64 i = b; i < e_; i++) {
            const u64 key = hkey[i];
            disco_contained_row &r = out[i];
            r.contained = hid[i];
            r.super = CKEY_SUPER(key);
            r.j = CKEY_J(key);
            r.type = disco_hit_type(CKEY_SUFFIX(key), CKEY_REV(key));
            r.len2 = hln[i] & 0xFFFFu;
            r.len1 = hln[i] >> 16;
            u32 orient, off;
            disco_map_type(r.type, r.len1, kk, r.j, &orient, &off); /* BG/OverlapGraph.cpp:428-434 */
            r.orient = orient;
            r.start = off;
        }
    });
    return (int64_t)nc;
}

/* the slot -> edge mapping of the last emission; null: dense (slot i is edge i) */
static const u8 *out_valid(const disco_ctx *c) { return c->out_dense ? nullptr : (const u8 *)c->d_out_valid.p; }
static const u64 *out_pos(const disco_ctx *c) { return c->out_dense ? nullptr : (const u64 *)c->d_out_pos.p; }

int64_t disco_fetch_edges(disco_ctx *c, disco_edge *out, uint64_t cap)
{
    DISCO_TRACE("disco_fetch_edges");
    if (!c) return DISCO_E_ARG;
    if (c->phase < 8) return fail(c, DISCO_E_STATE, "disco_fetch_edges: run disco_transitive_reduce first");
    HIPCHK(c, hipSetDevice(c->device));
    const u64 ne = c->n_out;
    if (!out) return (int64_t)ne;
    if (cap < ne) return fail(c, DISCO_E_ARG, "disco_fetch_edges: need room for %llu edges", (unsigned long long)ne);
    if (ne == 0) return 0;
    CHK(ensure_host_len(c));
    /* drop the unused chunk tails of the emission (into buffers the context keeps: two allocations of 0.4 GB per call cost more than the
     * copy), then copy out 12 bytes per edge — source as 32 bits, packed entry — chunk k into pinned staging memory (kept by the context)
     * while the host threads turn chunk k - 1 into disco_edge records; a copy into pageable memory ran at a third of the link's rate */
    /* (a dense emission has no tails to drop: the entries go out from where the emission put them, and only the sources are narrowed to
     * 32 bits for the link — no compaction kernel, no second buffer of entries) */
    if (c->out_dense) CHK(ensure(c, c->d_fetch_src, ne + ne / 8 + 1024));
    else CHK(ensure_group(c, ne, ne + ne / 8 + 1024, c->d_fetch_src, c->d_fetch_ent));
    u32 *csrc = c->d_fetch_src;
    const u64 *cent = c->out_dense ? (const u64 *)c->d_out_ent : (const u64 *)c->d_fetch_ent;
    if (c->out_dense) hipLaunchKernelGGL(emit_src32_kernel, dim3(flat_grid(c, ne)), dim3(256), 0, c->stream, c->d_out_src, ne, csrc);
    else hipLaunchKernelGGL(emit_compact32_kernel, dim3(flat_grid(c, c->out_used)), dim3(256), 0, c->stream, c->d_out_src, c->d_out_ent, c->d_out_valid, c->d_out_pos, c->out_used, csrc, c->d_fetch_ent.p);
    const u64 CHUNK = 1ull << 22; /* 4 M edges: 48 MB per half */
    if (!c->h_stage) {
        if (hipHostMalloc((void **)&c->h_stage, 4 * CHUNK * sizeof(u64)) != hipSuccess) c->h_stage = nullptr;
        for (int i = 0; i < 2 && c->h_stage; i++)
            if (hipEventCreateWithFlags(&c->ev_stage[i], hipEventDisableTiming) != hipSuccess) {
                (void)hipHostFree(c->h_stage);
                c->h_stage = nullptr;
            }
    }
    const u16 *hlen = c->h_len.data();
    auto convert = [&](const u32 *hsp, const u64 *hep, u64 base, u64 cnt) {
        parallel_for(cnt, [&, hlen, hsp, hep, base](u64 b, u64 e_) {
            for (u64 i = b; i < e_; i++) {
                disco_edge &e = out[base + i];
                e.src = hsp[i];
                e.dst = ADJ_DST(hep[i]);
                e.orient = ADJ_ORI(hep[i]);
                e.offset = ADJ_OFF(hep[i]);
                e.len_src = hlen[e.src];
                e.len_dst = ADJ_DLEN(hep[i]);
            }
        });
    };
    bool ok = true;
    if (c->h_stage) {
        const u64 nch = (ne + CHUNK - 1) / CHUNK;
        auto half_ent = [&](u64 k) { return c->h_stage + (k & 1) * 2 * CHUNK; };          /* entries: CHUNK words   */
        auto half_src = [&](u64 k) { return (u32 *)(c->h_stage + (k & 1) * 2 * CHUNK + CHUNK); }; /* sources: CHUNK / 2 words */
        auto issue = [&](u64 k) {
            const u64 cnt = std::min(CHUNK, ne - k * CHUNK);
            ok = ok && hipMemcpyAsync(half_src(k), csrc + k * CHUNK, cnt * 4, hipMemcpyDeviceToHost, c->stream) == hipSuccess &&
                 hipMemcpyAsync(half_ent(k), cent + k * CHUNK, cnt * 8, hipMemcpyDeviceToHost, c->stream) == hipSuccess &&
                 hipEventRecord(c->ev_stage[k & 1], c->stream) == hipSuccess;
        };
        issue(0);
        for (u64 k = 0; k < nch && ok; k++) {
            ok = hipEventSynchronize(c->ev_stage[k & 1]) == hipSuccess;
            if (k + 1 < nch) issue(k + 1); /* into the other half, converted one iteration ago */
            if (ok) convert(half_src(k), half_ent(k), k * CHUNK, std::min(CHUNK, ne - k * CHUNK));
        }
        ok = (hipStreamSynchronize(c->stream) == hipSuccess) && ok;
    } else { /* no pinned memory to be had: one pageable copy */
        std::unique_ptr<u32[]> hs(new u32[ne]);
        std::unique_ptr<u64[]> he(new u64[ne]); /* not zero-filled: 0.5 GB at 45 M edges */
        ok = hipMemcpyAsync(hs.get(), csrc, ne * 4, hipMemcpyDeviceToHost, c->stream) == hipSuccess &&
             hipMemcpyAsync(he.get(), cent, ne * 8, hipMemcpyDeviceToHost, c->stream) == hipSuccess && hipStreamSynchronize(c->stream) == hipSuccess;
        if (ok) convert(hs.get(), he.get(), 0, ne);
    }
    if (!ok) return fail(c, DISCO_E_HIP, "disco_fetch_edges: copy failed");
    return (int64_t)ne;
}

int64_t disco_fetch_edge_substitutions(disco_ctx *c, uint16_t *out, uint64_t cap)
{
    if (!c) return DISCO_E_ARG;
    if (c->phase < 8) return fail(c, DISCO_E_STATE, "disco_fetch_edge_substitutions: run disco_transitive_reduce first");
    HIPCHK(c, hipSetDevice(c->device));
    const u64 ne = c->n_out;
    if (!out) return (int64_t)ne;
    if (cap < ne) return fail(c, DISCO_E_ARG, "disco_fetch_edge_substitutions: need room for %llu edges", (unsigned long long)ne);
    if (ne == 0) return 0;
    if (c->prm.max_substitutions == 0) { /* exact overlaps: nothing to count */
        memset(out, 0, ne * sizeof(uint16_t));
        return (int64_t)ne;
    }
    LocalBuf<u16> subs(c);
    CHK(ensure(c, subs, ne));
    hipLaunchKernelGGL(edge_subs_kernel, dim3(flat_grid(c, c->out_used)), dim3(256), 0, c->stream, c->d_out_src, c->d_out_ent, out_valid(c), out_pos(c),
                       c->out_used, c->d_reads, c->d_len, c->S, subs);
    if (hipMemcpyAsync(out, subs, ne * sizeof(u16), hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
        return fail(c, DISCO_E_HIP, "disco_fetch_edge_substitutions: copy failed");
    return (int64_t)ne;
}

/* connected components of the edges in the slots [0, n_slots) (valid[i] != 0; pos[i] = rank of the edge among the valid ones)
 * dealt out to n_files files: out[pos[i]] = file of edge i — on the host, or, with d_out (room for ne entries), left on the device.
 * The assignment depends on the SET of edges only, not on their order or on who computes it: a component's root is its smallest read
 * (uf_hook_kernel), its size its number of edges, those of at least max(ne / (64 n_files), 1) edges are dealt out in (size descending,
 * root ascending) order to the lightest file (the lowest index among equals), the others by a hash of the root (tests/partition_model.py
 * is this rule in numpy, and tests/test_gpu_edge_partition.py holds the kernels to it) — which is what lets every rank of a multi-GPU
 * job run it on the gathered edges and arrive at the same files (disco_dist_format_edges) */
static int64_t partition_edges(disco_ctx *c, const u64 *d_src, const u64 *d_ent, const u8 *d_valid, const u64 *d_pos, u64 n_slots, u64 ne, u64 n,
                               uint32_t n_files, uint16_t *out, u16 *d_out = nullptr)
{
    DISCO_TRACE("partition_edges");
    LocalBuf<u32> parent(c), cnt(c), d_nlist(c);
    LocalBuf<u16> cfile(c), efile(c);
    LocalBuf<u64> list(c);
    /* components of at least 1/(64 files) of the edges are dealt out by size, largest first to the lightest file; the rest
     * (there can be millions of small ones) go by hash. ALL of the former: the list holds as many as there can be — min(n, ne / thr),
     * and ne / thr < 128 files — so that which of them are dealt out by size is never a matter of who arrived first */
    const u32 thr = (u32)std::max<u64>(ne / ((u64)n_files * 64), 1);
    const u32 list_cap = (u32)std::max<u64>(std::min<u64>(n, ne / thr), 1);
    CHK(ensure(c, parent, n));
    CHK(ensure(c, cnt, n));
    CHK(ensure(c, cfile, n));
    if (!d_out) CHK(ensure(c, efile, ne));
    CHK(ensure(c, list, list_cap));
    CHK(ensure(c, d_nlist, 1));
    hipLaunchKernelGGL(uf_init_kernel, dim3(flat_grid(c, n)), dim3(256), 0, c->stream, parent, n);
    hipLaunchKernelGGL(uf_hook_kernel, dim3(flat_grid(c, n_slots)), dim3(256), 0, c->stream, d_src, d_ent, d_valid, n_slots, parent);
    hipLaunchKernelGGL(uf_compress_kernel, dim3(flat_grid(c, n)), dim3(256), 0, c->stream, parent, n);
    (void)hipMemsetAsync(cnt, 0, n * sizeof(u32), c->stream);
    (void)hipMemsetAsync(cfile, 0xFF, n * sizeof(u16), c->stream);
    (void)hipMemsetAsync(d_nlist, 0, sizeof(u32), c->stream);
    hipLaunchKernelGGL(uf_count_kernel, dim3(flat_grid(c, n_slots)), dim3(256), 0, c->stream, d_src, d_valid, n_slots, parent, cnt);
    hipLaunchKernelGGL(uf_big_kernel, dim3(flat_grid(c, n)), dim3(256), 0, c->stream, cnt, n, thr, list, d_nlist, list_cap);
    u32 n_list = 0;
    if (hipMemcpyAsync(&n_list, d_nlist, sizeof(u32), hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
        return fail(c, DISCO_E_HIP, "edge partition: %s", hipGetErrorString(hipGetLastError()));
    if (n_list > list_cap) /* cannot happen (see list_cap); a clipped list would cut files that depend on the order of arrival */
        return fail(c, DISCO_E_CAPACITY, "edge partition: %u components of at least %u edges, room for %u", n_list, thr, list_cap);
    std::vector<u64> hl(n_list);
    if (n_list && (hipMemcpyAsync(hl.data(), list, n_list * sizeof(u64), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
                   hipStreamSynchronize(c->stream) != hipSuccess))
        return fail(c, DISCO_E_HIP, "edge partition: %s", hipGetErrorString(hipGetLastError()));
    std::sort(hl.begin(), hl.end(), [](u64 a, u64 b) { return (u32)a != (u32)b ? (u32)a > (u32)b : a < b; }); /* by size, then root: deterministic */
    /* the lightest file, the lowest index among equals: a heap of (load, file) — the list can hold 128 entries per file */
    typedef std::pair<u64, u32> LoadOfFile;
    std::priority_queue<LoadOfFile, std::vector<LoadOfFile>, std::greater<LoadOfFile>> lightest;
    for (u32 f = 0; f < n_files; f++) lightest.push(LoadOfFile(0, f));
    for (u64 &e : hl) {
        const LoadOfFile t = lightest.top();
        lightest.pop();
        lightest.push(LoadOfFile(t.first + (u32)e, t.second));
        e = (e & 0xFFFFFFFF00000000ull) | t.second;
    }
    if (n_list) {
        if (hipMemcpyAsync(list, hl.data(), n_list * sizeof(u64), hipMemcpyHostToDevice, c->stream) != hipSuccess) return fail(c, DISCO_E_HIP, "edge partition: upload failed");
        hipLaunchKernelGGL(uf_assign_kernel, dim3((n_list + 255) / 256), dim3(256), 0, c->stream, list, n_list, cfile);
    }
    hipLaunchKernelGGL(uf_edge_file_kernel, dim3(flat_grid(c, n_slots)), dim3(256), 0, c->stream, d_src, d_valid, d_pos, n_slots, parent, cfile, n_files, d_out ? d_out : efile.p);
    if ((d_out ? hipGetLastError() : hipMemcpyAsync(out, efile, ne * sizeof(u16), hipMemcpyDeviceToHost, c->stream)) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
        return fail(c, DISCO_E_HIP, "edge partition: copy failed");
    return (int64_t)ne;
}

int64_t disco_fetch_edge_files(disco_ctx *c, uint32_t n_files, uint16_t *out, uint64_t cap)
{
    DISCO_TRACE("disco_fetch_edge_files");
    if (!c || !out || n_files == 0) return DISCO_E_ARG;
    if (n_files > 0xFFFEu) return fail(c, DISCO_E_ARG, "disco_fetch_edge_files: at most 65534 files (%u asked for)", n_files);
    if (c->phase < 8) return fail(c, DISCO_E_STATE, "disco_fetch_edge_files: run disco_transitive_reduce first");
    HIPCHK(c, hipSetDevice(c->device));
    const u64 ne = c->n_out;
    if (cap < ne) return fail(c, DISCO_E_ARG, "disco_fetch_edge_files: need room for %llu edges", (unsigned long long)ne);
    if (ne == 0) return 0;
    return partition_edges(c, c->d_out_src, c->d_out_ent, out_valid(c), out_pos(c), c->out_used, ne, c->n, n_files, out);
}

/* the same partition for edges held by the HOST (buildG --gpus N: the edges of all ranks, concatenated): src / dst are read ids
 * below n_nodes */
int64_t disco_partition_edges(disco_ctx *c, const disco_edge *edges, uint64_t n_edges, uint64_t n_nodes, uint32_t n_files, uint16_t *out)
{
    if (!c || !out || n_files == 0 || (n_edges && !edges)) return DISCO_E_ARG;
    if (n_files > 0xFFFEu) return fail(c, DISCO_E_ARG, "disco_partition_edges: at most 65534 files (%u asked for)", n_files);
    if (n_nodes >= (1ull << 31)) return fail(c, DISCO_E_UNSUPPORTED, "disco_partition_edges: more than 2^31 nodes");
    HIPCHK(c, hipSetDevice(c->device));
    if (n_edges == 0) return 0;
    LocalBuf<u64> d_src(c), d_ent(c), d_pos(c);
    LocalBuf<u8> d_valid(c);
    std::unique_ptr<u64[]> hs(new u64[n_edges]), he(new u64[n_edges]);
    parallel_for(n_edges, [&](u64 b, u64 e_) {
        for (u64 i = b; i < e_; i++) {
            hs[i] = edges[i].src;
            he[i] = ADJ_MAKE(0u, edges[i].dst, 0u, 0u);
        }
    });
    CHK(ensure(c, d_src, n_edges));
    CHK(ensure(c, d_ent, n_edges));
    CHK(ensure(c, d_pos, n_edges));
    CHK(ensure(c, d_valid, n_edges));
    if (hipMemcpyAsync(d_src, hs.get(), n_edges * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync(d_ent, he.get(), n_edges * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess || hipMemsetAsync(d_valid, 1, n_edges, c->stream) != hipSuccess)
        return fail(c, DISCO_E_HIP, "disco_partition_edges: upload failed");
    hipLaunchKernelGGL(iota_u64_kernel, dim3(flat_grid(c, n_edges)), dim3(256), 0, c->stream, d_pos, n_edges);
    return partition_edges(c, d_src, d_ent, d_valid, d_pos, n_edges, n_edges, n_nodes, n_files, out);
}

/* ---- the edge lines of the text files, formatted where the edges are (disco_text.h) ------------------------------------------ */
/* every line measured (bytes[ne]), then the lines of the files [f_lo, f_hi) placed, file behind file: place[i] = where the line of edge i
 * begins in the text, off[f] = where file f does (a file outside the range is empty), off[n_files] = all bytes. One GPU: every file; a
 * rank of a multi-GPU job: its own. sel / within: scratch of ne and ne + 1 elements (not touched when the range is empty) */
static int place_edge_lines(disco_ctx *c, const TextView &g, u64 ne, const u16 *efile, uint32_t n_files, uint32_t f_lo, uint32_t f_hi, u8 *bytes, u8 *sel, u64 *within, u64 *place,
                            uint64_t *off)
{
    hipLaunchKernelGGL(text_measure_kernel, dim3(flat_grid(c, g.n_slots)), dim3(256), 0, c->stream, g, bytes);
    u64 base = 0;
    for (uint32_t f = 0; f < n_files; f++) {
        off[f] = base;
        if (f < f_lo || f >= f_hi) continue;
        u64 total = 0;
        hipLaunchKernelGGL(text_select_kernel, dim3(flat_grid(c, ne)), dim3(256), 0, c->stream, (const u8 *)bytes, efile, ne, f, sel);
        CHK((scan_exclusive<u8, u64>(c, sel, ne, within, false, &total)));
        hipLaunchKernelGGL(text_place_kernel, dim3(flat_grid(c, ne)), dim3(256), 0, c->stream, (const u64 *)within, efile, ne, f, base, place);
        base += total;
    }
    off[n_files] = base;
    return DISCO_OK;
}

int64_t disco_format_edges(disco_ctx *c, uint32_t n_files, const uint16_t *edge_file, const uint64_t *file_index, uint64_t *file_offsets)
{
    DISCO_TRACE("disco_format_edges");
    if (!c || !file_offsets || n_files == 0) return DISCO_E_ARG;
    if (c->phase < 8) return fail(c, DISCO_E_STATE, "disco_format_edges: run disco_transitive_reduce first");
    if (n_files > 256) return fail(c, DISCO_E_UNSUPPORTED, "disco_format_edges: more than 256 files (one placement pass per file)");
    if (c->prm.max_substitutions) return fail(c, DISCO_E_UNSUPPORTED, "disco_format_edges: the substitutions column is written by the host writer");
    HIPCHK(c, hipSetDevice(c->device));
    const u64 ne = c->n_out;
    for (uint32_t f = 0; f <= n_files; f++) file_offsets[f] = 0;
    c->text.bytes = 0;
    if (ne == 0) return 0;
    if (!edge_file && n_files > 1) return fail(c, DISCO_E_ARG, "disco_format_edges: the file of every edge is needed for more than one file");
    TextView g;
    g.src = c->d_out_src;
    g.ent = c->d_out_ent;
    g.valid = out_valid(c);
    g.pos = out_pos(c);
    g.len = c->d_len;
    g.n_slots = c->out_used;
    LocalBuf<u64> d_findex(c), within(c), place(c);
    LocalBuf<u8> bytes(c), sel(c);
    LocalBuf<u16> efile(c);
    if (file_index) {
        CHK(ensure(c, d_findex, c->n));
        HIPCHK(c, hipMemcpyAsync(d_findex, file_index, c->n * 8, hipMemcpyHostToDevice, c->stream));
    }
    g.file_index = d_findex;
    CHK(ensure(c, bytes, ne));
    CHK(ensure(c, sel, ne));
    CHK(ensure(c, efile, ne));
    CHK(ensure(c, within, ne + 1));
    CHK(ensure(c, place, ne));
    if (edge_file) HIPCHK(c, hipMemcpyAsync(efile, edge_file, ne * sizeof(u16), hipMemcpyHostToDevice, c->stream));
    else HIPCHK(c, hipMemsetAsync(efile, 0, ne * sizeof(u16), c->stream));
    CHK(place_edge_lines(c, g, ne, efile, n_files, 0, n_files, bytes, sel, within, place, file_offsets));
    const u64 base = file_offsets[n_files];
    c->text.off.assign(file_offsets, file_offsets + n_files + 1);
    CHK(ensure(c, c->text.d, std::max<u64>(base, 1)));
    hipLaunchKernelGGL(text_write_kernel, dim3(flat_grid(c, g.n_slots)), dim3(256), 0, c->stream, g, place, c->text.d);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->text.bytes = base;
    return (int64_t)c->text.bytes;
}

/* a text into the caller's memory */
static int fetch_text(disco_ctx *c, const char *who, const TextProduct &t, char *out, uint64_t cap)
{
    if (!out && t.bytes) return DISCO_E_ARG;
    if (cap < t.bytes) return fail(c, DISCO_E_ARG, "%s: need room for %llu bytes", who, (unsigned long long)t.bytes);
    HIPCHK(c, hipSetDevice(c->device));
    if (t.bytes) {
        HIPCHK(c, hipMemcpyAsync(out, t.d, t.bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return DISCO_OK;
}

int disco_fetch_edge_text(disco_ctx *c, char *out, uint64_t cap) { return c ? fetch_text(c, "disco_fetch_edge_text", c->text, out, cap) : DISCO_E_ARG; }

/* Everything that leaves the device through the pinned ring: piece k is copied into half k & 1 of the ring and, while it travels, the
 * host delivers piece k - 1 to where it belongs (disco_ringio.h) — the mirror image of disco_ingest_fasta's file reader. A piece is
 * one or more parts, each with a place in the half and a destination; the two device buffers pieces are formed in are the sink's
 * (home: the context keeps them between calls). Kernel and copy share the stream: 128 MB are formed in a fraction of a millisecond and
 * travel for several, so there is nothing a second stream could hide (profiles/binary_records.txt). */
struct RingPart {
    const void *d_src; /* on the device */
    size_t at, len;    /* [at, at + len) of the half */
    int fd;            /* the file ... */
    char *host;        /* ... or, not null, the caller's memory */
    u64 off;           /* where the bytes belong there */
};
struct RingSink {
    disco_ctx *const c;
    const char *const who;
    DevBuf<u8> *const home;
    LocalBuf<u8> piece[2];
    u64 issued = 0; /* pieces so far */
    std::vector<ringio::Segment> pending; /* the piece before the current one lies in its half, not yet delivered */
    unsigned pending_split = 0;
    bool write_ok = true;

    RingSink(disco_ctx *ctx, const char *w, DevBuf<u8> *keep = nullptr) : c(ctx), who(w), home(keep), piece{LocalBuf<u8>(ctx), LocalBuf<u8>(ctx)}
    {
        for (int i = 0; home && i < 2; i++) piece[i].take(home[i]);
    }
    ~RingSink()
    {
        for (int i = 0; home && i < 2; i++) piece[i].give(home[i]);
    }
    u8 *next() const { return piece[issued & 1].p; } /* where the next piece is formed */
    void deliver()
    {
        bool ok = true;
        if (pending_split) {
            for (const ringio::Segment &s : pending) ok = ringio::deliver_split(s, pending_split) && ok;
        } else
            ok = ringio::deliver_each(pending.data(), pending.size());
        pending.clear();
        if (!ok) write_ok = false;
    }
    /* the next piece: its parts travel into their half while the host delivers the piece before — split: every part among that many
     * writers (the bytes of ONE file); 0: one writer per part (writes to one file serialise on its inode lock — 16 threads on one
     * file: 12 GB/s; one thread on each of 16 files: the link's rate) */
    int ship(const RingPart *parts, size_t n, unsigned split)
    {
        const u64 k = issued & 1;
        char *half = (char *)c->h_ring + k * c->ring_half;
        for (size_t i = 0; i < n; i++)
            if (parts[i].len) HIPCHK(c, hipMemcpyAsync(half + parts[i].at, parts[i].d_src, parts[i].len, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipEventRecord(c->ev_ring[k], c->stream));
        deliver(); /* (its copies were waited for below, one piece ago; the half it frees is written again two pieces on) */
        HIPCHK(c, hipEventSynchronize(c->ev_ring[k]));
        for (size_t i = 0; i < n; i++) {
            ringio::Segment s;
            s.src = half + parts[i].at;
            s.len = parts[i].len;
            s.fd = parts[i].fd;
            s.host = parts[i].host;
            s.off = parts[i].off;
            pending.push_back(s);
        }
        pending_split = split;
        issued++;
        return DISCO_OK;
    }
    /* ... the piece of `bytes` bytes just launched into next() */
    int ship_piece(u64 bytes, int fd, void *host, u64 off, unsigned split)
    {
        HIPCHK(c, hipGetLastError());
        const RingPart p = {next(), 0, (size_t)bytes, fd, (char *)host, off};
        return ship(&p, 1, split);
    }
    int flush()
    {
        deliver();
        if (!write_ok) return fail(c, DISCO_E_ARG, "%s: write error", who);
        return DISCO_OK;
    }
};

/* formatted lines straight into the caller's open files (fds[f] receives the bytes of file f, from its offset 0), in rounds of up to
 * 128 MB. (disco_fetch_edge_text into 2.5 GB of fresh pageable memory, then the writer: 0.19 s at config 3; this: the link's 0.05 s.)
 * d_text: the files' text one behind the other, off: n_files + 1 offsets into it */
static int write_text(disco_ctx *c, const char *who, const char *formatter, const TextProduct &t, const int *fds, uint32_t n_files)
{
    if (!fds) return DISCO_E_ARG;
    if (t.off.size() != (size_t)n_files + 1) return fail(c, DISCO_E_STATE, "%s: run %s for %u files first", who, formatter, n_files);
    HIPCHK(c, hipSetDevice(c->device));
    if (t.bytes == 0) return DISCO_OK;
    const char *d_text = t.d;
    const std::vector<u64> &off = t.off;
    CHK(pinned_ring(c, who));
    /* a round moves one slice of every file: slice r of file f = bytes [r S, (r + 1) S) of it, S = the ring half divided among the files */
    const size_t S = (RING_HALF / n_files) & ~(size_t)4095;
    if (S == 0) return fail(c, DISCO_E_UNSUPPORTED, "%s: too many files for the staging ring", who);
    u64 longest = 0;
    for (uint32_t f = 0; f < n_files; f++) longest = std::max(longest, off[f + 1] - off[f]);
    const u64 rounds = (longest + S - 1) / S;
    RingSink o(c, who);
    std::vector<RingPart> parts(n_files);
    for (u64 r = 0; r < rounds; r++) {
        for (uint32_t f = 0; f < n_files; f++) {
            const u64 fl = off[f + 1] - off[f], lo = std::min<u64>(r * S, fl); /* file-local byte range of the slice */
            parts[f] = {d_text + off[f] + lo, (size_t)f * S, (size_t)(std::min<u64>((r + 1) * S, fl) - lo), fds[f], nullptr, lo};
        }
        CHK(o.ship(parts.data(), n_files, 0));
    }
    return o.flush();
}

int disco_write_edge_text(disco_ctx *c, const int *fds, uint32_t n_files, uint32_t)
{
    DISCO_TRACE("disco_write_edge_text");
    return c ? write_text(c, "disco_write_edge_text", "disco_format_edges", c->text, fds, n_files) : DISCO_E_ARG;
}

/* ---- the lines of the contained-read files, grouped, sorted and formatted where the keys are (disco_text.h) ------------------ */
/* the body of disco_format_contained and disco_dist_format_contained: the rows of the containing reads [s_lo, s_hi) out of best[0, n).
 * flags != null: the contained reads are the flagged ones and nc of them have a containing read in the range (one GPU: all of them,
 * known since disco_mark_contained); flags == null: read off the keys, counted here (a rank of a multi-GPU job) */
/* The contained rows of the containing reads [s_lo, s_hi), grouped by containing read and every group sorted — steps 1 and 2 of the text of
 * the contained-read files, which the records of the binary side output (disco_prepare_contained_records) take too: afterwards row i is
 * word[i] (CWORD_MAKE: j, contained read, suffix, rev) under the containing read sup[i], ascending (containing read, j, contained read),
 * gend[s] the end of the group of read s, ctr the figures of the sorts and the count of keys that name no read. The launches are on
 * c->stream and not waited for; the buffers go with G. *nc: in — the number of rows where flags are given; out — the rows of
 * the range where they are not (0: nothing was placed or sorted) */
struct ContainedGroups {
    LocalBuf<u32> cnt, gend, sup, list, ctr;
    LocalBuf<u64> word;
    explicit ContainedGroups(disco_ctx *c) : cnt(c), gend(c), sup(c), list(c), ctr(c), word(c) {}
};
static int group_contained_rows(disco_ctx *c, const u8 *flags, u64 s_lo, u64 s_hi, u64 *nc_io, ContainedGroups &G)
{
    const u64 n = c->n;
    u64 nc = *nc_io;
    DevBuf<u32> &cnt = G.cnt, &gend = G.gend, &sup = G.sup, &list = G.list, &ctr = G.ctr;
    DevBuf<u64> &word = G.word;
    /* 1. grouped by containing read */
    CHK(ensure(c, cnt, n + 1));
    CHK(ensure(c, gend, n + 1));
    CHK(ensure(c, ctr, CGRP_CTRS));
    HIPCHK(c, hipMemsetAsync(cnt, 0, (n + 1) * sizeof(u32), c->stream));
    HIPCHK(c, hipMemsetAsync(ctr, 0, CGRP_CTRS * sizeof(u32), c->stream));
    if (flags) {
        hipLaunchKernelGGL(cgrp_count_kernel, dim3(flat_grid(c, n)), dim3(256), 0, c->stream, (const u64 *)c->d_best, flags, n, cnt.p, ctr.p);
        CHK((scan_exclusive<u32, u32>(c, cnt, n + 1, gend, false, nullptr)));
    } else {
        hipLaunchKernelGGL(cgrp_count_range_kernel, dim3(flat_grid(c, n)), dim3(256), 0, c->stream, (const u64 *)c->d_best, n, s_lo, s_hi, cnt.p, ctr.p);
        CHK((scan_exclusive<u32, u32>(c, cnt, n + 1, gend, false, &nc))); /* (the rank's rows: known only now) */
        *nc_io = nc;
        if (nc == 0) return DISCO_OK;
    }
    CgrpLists L;
    L.cap = (u32)(nc / (CROW_GROUP_MAX + 1) + 1); /* (a listed group has more than CROW_GROUP_MAX rows) */
    CHK(ensure(c, word, nc));
    CHK(ensure(c, sup, nc));
    CHK(ensure(c, list, 2 * (u64)L.cap));
    L.lds = list;
    L.glb = list.p + L.cap;
    L.ctr = ctr;
    if (flags) hipLaunchKernelGGL(cgrp_place_kernel, dim3(flat_grid(c, n)), dim3(256), 0, c->stream, (const u64 *)c->d_best, flags, n, nc, gend.p, word.p, sup.p);
    else hipLaunchKernelGGL(cgrp_place_range_kernel, dim3(flat_grid(c, n)), dim3(256), 0, c->stream, (const u64 *)c->d_best, n, s_lo, s_hi, nc, gend.p, word.p, sup.p);
    /* 2. every group in (j, contained read) order: by its size */
    hipLaunchKernelGGL(cgrp_sort_small_kernel, dim3(flat_grid(c, n)), dim3(256), 0, c->stream, (const u32 *)gend, n, word.p, L);
    const int big_grid = (int)std::min<u64>(L.cap, (u64)c->n_cu * 4);
    hipLaunchKernelGGL(cgrp_sort_lds_kernel, dim3(big_grid), dim3(CGRP_BLOCK), 0, c->stream, (const u32 *)gend, word.p, L);
    hipLaunchKernelGGL(cgrp_sort_global_kernel, dim3(big_grid), dim3(CGRP_BLOCK), 0, c->stream, (const u32 *)gend, word.p, L);
    HIPCHK(c, hipGetLastError());
    release(c, cnt); /* (only the grouping needed it: not held while the caller formats) */
    return DISCO_OK;
}

static int64_t format_contained_rows(disco_ctx *c, const char *who, uint32_t n_files, const uint64_t *file_index, uint64_t *file_offsets, const u8 *flags, u64 s_lo,
                                     u64 s_hi, u64 nc)
{
    const u64 n = c->n;
    ContainedGroups G(c);
    DevBuf<u32> &gend = G.gend, &sup = G.sup, &ctr = G.ctr;
    DevBuf<u64> &word = G.word;
    LocalBuf<u64> place(c), d_findex(c), d_off(c);
    LocalBuf<u8> bytes(c);
    u32 h_ctr[CGRP_CTRS] = {0, 0, 0, 0};
    /* 1., 2. grouped by containing read, every group in (j, contained read) order */
    CHK(group_contained_rows(c, flags, s_lo, s_hi, &nc, G));
    if (nc) {
        /* 3. measure -> scan -> write; the context's offsets (all 0 since the caller began) change only once the text is there */
        std::vector<u64> off((size_t)n_files + 1, 0);
        CTextView g;
        g.word = word;
        g.sup = sup;
        g.len = c->d_len;
        g.nc = nc;
        g.k = (u32)c->k;
        if (file_index) {
            CHK(ensure(c, d_findex, n));
            HIPCHK(c, hipMemcpyAsync(d_findex, file_index, n * 8, hipMemcpyHostToDevice, c->stream));
        }
        g.file_index = d_findex;
        CHK(ensure(c, bytes, nc));
        CHK(ensure(c, place, nc + 1));
        CHK(ensure(c, d_off, (u64)n_files + 1));
        hipLaunchKernelGGL(ctext_measure_kernel, dim3(flat_grid(c, nc)), dim3(256), 0, c->stream, g, bytes.p);
        u64 total = 0;
        CHK((scan_exclusive<u8, u64>(c, bytes, nc, place, true, &total)));
        hipLaunchKernelGGL(ctext_offsets_kernel, dim3(flat_grid(c, (u64)n_files + 1)), dim3(256), 0, c->stream, (const u32 *)gend, n, nc, (const u64 *)place, n_files, d_off.p);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(off.data(), d_off, ((size_t)n_files + 1) * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(h_ctr, ctr, sizeof h_ctr, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (h_ctr[CGRP_BAD_KEYS]) return fail(c, DISCO_E_STATE, "%s: %u contained reads have a key that names no containing read", who, h_ctr[CGRP_BAD_KEYS]);
        CHK(ensure(c, c->ctext.d, std::max<u64>(total, 1)));
        hipLaunchKernelGGL(ctext_write_kernel, dim3(flat_grid(c, nc)), dim3(256), 0, c->stream, g, (const u64 *)place, c->ctext.d.p);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->ctext.off.swap(off);
        c->ctext.bytes = total;
    }
    for (uint32_t f = 0; f <= n_files; f++) file_offsets[f] = c->ctext.off[f];
    if (getenv("DISCO_VERBOSE"))
        fprintf(stderr, "[disco] contained lines: %llu rows, %llu bytes; groups of more than %d rows: %u sorted in LDS, %u through global memory, the largest of %u rows\n",
                (unsigned long long)nc, (unsigned long long)c->ctext.bytes, CROW_GROUP_MAX, h_ctr[CGRP_N_LDS], h_ctr[CGRP_N_GLOBAL], h_ctr[CGRP_LARGEST]);
    return (int64_t)c->ctext.bytes;
}

int64_t disco_format_contained(disco_ctx *c, uint32_t n_files, const uint64_t *file_index, uint64_t *file_offsets)
{
    DISCO_TRACE("disco_format_contained");
    if (!c || !file_offsets || n_files == 0) return DISCO_E_ARG;
    if (c->comm) return fail(c, DISCO_E_UNSUPPORTED, "disco_format_contained: a rank's rows are not grouped across ranks (the host writer formats)");
    if (c->phase < 4) return fail(c, DISCO_E_STATE, "disco_format_contained: run disco_mark_contained first");
    if (c->n >= (1ull << 31)) return fail(c, DISCO_E_UNSUPPORTED, "disco_format_contained: more than 2^31 reads");
    HIPCHK(c, hipSetDevice(c->device));
    for (uint32_t f = 0; f <= n_files; f++) file_offsets[f] = 0;
    c->ctext.bytes = 0;
    c->ctext.off.assign((size_t)n_files + 1, 0);
    if (c->n_contained == 0) return 0;
    CHK(settle_keys(c));
    return format_contained_rows(c, "disco_format_contained", n_files, file_index, file_offsets, (const u8 *)c->d_contained, 0, c->n, c->n_contained);
}

int disco_fetch_contained_text(disco_ctx *c, char *out, uint64_t cap) { return c ? fetch_text(c, "disco_fetch_contained_text", c->ctext, out, cap) : DISCO_E_ARG; }

int disco_write_contained_text(disco_ctx *c, const int *fds, uint32_t n_files, uint32_t)
{
    DISCO_TRACE("disco_write_contained_text");
    return c ? write_text(c, "disco_write_contained_text", "disco_format_contained", c->ctext, fds, n_files) : DISCO_E_ARG;
}

/* ---- the records of the binary side output, formed where the edges and the keys are (disco_binrec.h) ------------------------- */
/* The records [0, total) of one kind leave the device piece by piece: launch(lo, hi, piece) fills a device piece buffer with the records
 * [lo, hi), and the pieces go through a RingSink to `out` or (out == null) into fd from file_offset on, a piece split among `threads`
 * writers: the records of a kind lie in ONE file. No device buffer holds all records. */
static int records_through_ring(disco_ctx *c, const char *who, u64 total, const std::function<void(u64, u64, u64 *)> &launch, void *out, int fd, u64 file_offset,
                                uint32_t threads)
{
    if (total == 0) return DISCO_OK;
    CHK(pinned_ring(c, who));
    const u64 REC = BINREC_WORDS * sizeof(u64);
    const u64 fits = c->ring_half / REC;
    const u64 P = std::min<u64>(c->rec_piece ? std::min<u64>(c->rec_piece, fits) : fits, total);
    const u64 pieces = (total + P - 1) / P;
    RingSink o(c, who, c->d_rec_piece);
    for (u64 i = 0; i < std::min<u64>(pieces, 2); i++) CHK(ensure(c, o.piece[i], P * REC));
    for (u64 lo = 0; lo < total; lo += P) {
        const u64 hi = std::min(total, lo + P);
        launch(lo, hi, (u64 *)o.next());
        CHK(o.ship_piece((hi - lo) * REC, fd, out, (out ? 0 : file_offset) + lo * REC, std::max<uint32_t>(threads, 1)));
    }
    return o.flush();
}

static int records_common_checks(disco_ctx *c, const char *who, int phase_needed, const char *phase_name)
{
    if (c->comm) return fail(c, DISCO_E_UNSUPPORTED, "%s: a rank holds its share of the job only (the host writer takes the gathered records)", who);
    if (c->n >= (1ull << 31)) return fail(c, DISCO_E_UNSUPPORTED, "%s: more than 2^31 reads", who);
    if (c->phase < phase_needed) return fail(c, DISCO_E_STATE, "%s: run %s first", who, phase_name);
    return DISCO_OK;
}

/* what the edge records need next to the edges: the caller's arrays and the substitution counts, kept in the context */
static int edge_record_inputs(disco_ctx *c, const uint16_t *edge_file, const uint64_t *file_index)
{
    const u64 ne = c->n_out;
    if (edge_file) {
        CHK(ensure(c, c->d_rec_efile, ne));
        HIPCHK(c, hipMemcpyAsync(c->d_rec_efile, edge_file, ne * sizeof(u16), hipMemcpyHostToDevice, c->stream));
        c->rec_e_has_file = true;
    }
    if (file_index) {
        CHK(ensure(c, c->d_rec_efindex, c->n));
        HIPCHK(c, hipMemcpyAsync(c->d_rec_efindex, file_index, c->n * 8, hipMemcpyHostToDevice, c->stream));
        c->rec_e_has_findex = true;
    }
    if (c->prm.max_substitutions) { /* by fetch-order rank, as disco_fetch_edge_substitutions has them */
        CHK(ensure(c, c->d_rec_subs, ne));
        hipLaunchKernelGGL(edge_subs_kernel, dim3(flat_grid(c, c->out_used)), dim3(256), 0, c->stream, c->d_out_src, c->d_out_ent, out_valid(c), out_pos(c), c->out_used,
                           c->d_reads, c->d_len, c->S, c->d_rec_subs.p);
        HIPCHK(c, hipGetLastError());
        c->rec_e_has_subs = true;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream)); /* (the caller's arrays are free again) */
    return DISCO_OK;
}

/* replaces the edge half of disco::write_binary (disco_amd/host/writer.h; the records of the lines of BG/OverlapGraph.cpp:808-867) */
int64_t disco_prepare_edge_records(disco_ctx *c, uint32_t n_files, const uint16_t *edge_file, const uint64_t *file_index)
{
    DISCO_TRACE("disco_prepare_edge_records");
    if (!c || n_files == 0) return DISCO_E_ARG;
    if (n_files > 0xFFFEu) return fail(c, DISCO_E_ARG, "disco_prepare_edge_records: at most 65534 files (%u asked for)", n_files);
    CHK(records_common_checks(c, "disco_prepare_edge_records", 8, "disco_transitive_reduce"));
    if (!edge_file && n_files > 1) return fail(c, DISCO_E_ARG, "disco_prepare_edge_records: the file of every edge is needed for more than one file");
    HIPCHK(c, hipSetDevice(c->device));
    drop_edge_records(c);
    c->rec_e_files = n_files;
    c->rec_e_has_file = c->rec_e_has_findex = c->rec_e_has_subs = false;
    const int rc = c->n_out ? edge_record_inputs(c, edge_file, file_index) : DISCO_OK;
    if (rc != DISCO_OK) {
        drop_edge_records(c);
        return rc;
    }
    c->rec_e_ready = true;
    return (int64_t)c->n_out;
}

static int edge_records_out(disco_ctx *c, const char *who, void *out, int fd, u64 file_offset, uint32_t threads)
{
    if (!c->rec_e_ready || c->phase < 8) return fail(c, DISCO_E_STATE, "%s: run disco_prepare_edge_records first", who);
    HIPCHK(c, hipSetDevice(c->device));
    const u64 ne = c->n_out;
    if (ne == 0) return DISCO_OK;
    BinEdgeView g{};
    if (c->out_dense) {
        g.src64 = c->d_out_src;
        g.ent = c->d_out_ent;
    } else { /* an emission with unused chunk tails: through disco_fetch_edges's compaction, so that slot i is edge i */
        CHK(ensure_group(c, ne, ne + ne / 8 + 1024, c->d_fetch_src, c->d_fetch_ent));
        hipLaunchKernelGGL(emit_compact32_kernel, dim3(flat_grid(c, c->out_used)), dim3(256), 0, c->stream, c->d_out_src, c->d_out_ent, c->d_out_valid, c->d_out_pos, c->out_used,
                           c->d_fetch_src.p, c->d_fetch_ent.p);
        HIPCHK(c, hipGetLastError());
        g.src32 = c->d_fetch_src;
        g.ent = c->d_fetch_ent;
    }
    g.len = c->d_len;
    g.file_index = c->rec_e_has_findex ? c->d_rec_efindex.p : nullptr;
    g.edge_file = c->rec_e_has_file ? c->d_rec_efile.p : nullptr;
    g.subs = c->rec_e_has_subs ? c->d_rec_subs.p : nullptr;
    g.n_files = c->rec_e_files;
    return records_through_ring(
        c, who, ne, [&](u64 lo, u64 hi, u64 *piece) { hipLaunchKernelGGL(binrec_edges_kernel, dim3(flat_grid(c, hi - lo)), dim3(256), 0, c->stream, g, lo, hi, piece); }, out, fd,
        file_offset, threads);
}

int disco_fetch_edge_records(disco_ctx *c, disco_bin_edge *out, uint64_t cap)
{
    DISCO_TRACE("disco_fetch_edge_records");
    if (!c) return DISCO_E_ARG;
    if (c->rec_e_ready && c->phase >= 8 && c->n_out && (!out || cap < c->n_out))
        return fail(c, DISCO_E_ARG, "disco_fetch_edge_records: need room for %llu records", (unsigned long long)c->n_out);
    return edge_records_out(c, "disco_fetch_edge_records", out, -1, 0, 16);
}

int disco_write_edge_records(disco_ctx *c, int fd, uint64_t file_offset, uint32_t host_threads)
{
    DISCO_TRACE("disco_write_edge_records");
    if (!c || fd < 0) return DISCO_E_ARG;
    return edge_records_out(c, "disco_write_edge_records", nullptr, fd, file_offset, host_threads);
}

/* the contained rows grouped and sorted, and the caller's array: the rows stay with the context, the rest of the grouping goes */
static int contained_record_inputs(disco_ctx *c, const uint64_t *file_index, u64 *nc)
{
    ContainedGroups G(c);
    u32 h_ctr[CGRP_CTRS] = {0, 0, 0, 0};
    CHK(group_contained_rows(c, (const u8 *)c->d_contained, 0, c->n, nc, G));
    if (file_index) {
        CHK(ensure(c, c->d_rec_cfindex, c->n));
        HIPCHK(c, hipMemcpyAsync(c->d_rec_cfindex, file_index, c->n * 8, hipMemcpyHostToDevice, c->stream));
        c->rec_c_has_findex = true;
    }
    HIPCHK(c, hipMemcpyAsync(h_ctr, G.ctr, sizeof h_ctr, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (h_ctr[CGRP_BAD_KEYS]) return fail(c, DISCO_E_STATE, "disco_prepare_contained_records: %u contained reads have a key that names no containing read", h_ctr[CGRP_BAD_KEYS]);
    G.word.give(c->d_rec_cword); /* (empty since drop_contained_records; the bytes stay counted) */
    G.sup.give(c->d_rec_csup);
    return DISCO_OK;
}

/* replaces the contained half of disco::write_binary (disco_amd/host/writer.h; the records of the lines of BG/OverlapGraph.cpp:438-447) */
int64_t disco_prepare_contained_records(disco_ctx *c, uint32_t n_files, const uint64_t *file_index)
{
    DISCO_TRACE("disco_prepare_contained_records");
    if (!c || n_files == 0) return DISCO_E_ARG;
    if (n_files > 0xFFFEu) return fail(c, DISCO_E_ARG, "disco_prepare_contained_records: at most 65534 files (%u asked for)", n_files);
    CHK(records_common_checks(c, "disco_prepare_contained_records", 4, "disco_mark_contained"));
    HIPCHK(c, hipSetDevice(c->device));
    drop_contained_records(c);
    c->rec_c_files = n_files;
    c->rec_c_has_findex = false;
    u64 nc = c->n_contained;
    if (nc == 0) {
        c->rec_c_ready = true;
        return 0;
    }
    CHK(settle_keys(c));
    const int rc = contained_record_inputs(c, file_index, &nc);
    if (rc != DISCO_OK) {
        drop_contained_records(c);
        return rc;
    }
    c->rec_c_n = nc;
    c->rec_c_ready = true;
    return (int64_t)nc;
}

static int contained_records_out(disco_ctx *c, const char *who, void *out, int fd, u64 file_offset, uint32_t threads)
{
    if (!c->rec_c_ready || c->phase < 4) return fail(c, DISCO_E_STATE, "%s: run disco_prepare_contained_records first", who);
    HIPCHK(c, hipSetDevice(c->device));
    if (c->rec_c_n == 0) return DISCO_OK;
    CTextView g;
    g.word = c->d_rec_cword;
    g.sup = c->d_rec_csup;
    g.len = c->d_len;
    g.file_index = c->rec_c_has_findex ? c->d_rec_cfindex.p : nullptr;
    g.nc = c->rec_c_n;
    g.k = (u32)c->k;
    const u64 n = c->n;
    const u32 nf = c->rec_c_files;
    return records_through_ring(
        c, who, c->rec_c_n,
        [&](u64 lo, u64 hi, u64 *piece) { hipLaunchKernelGGL(binrec_contained_kernel, dim3(flat_grid(c, hi - lo)), dim3(256), 0, c->stream, g, n, nf, lo, hi, piece); }, out, fd,
        file_offset, threads);
}

int disco_fetch_contained_records(disco_ctx *c, disco_bin_contained *out, uint64_t cap)
{
    DISCO_TRACE("disco_fetch_contained_records");
    if (!c) return DISCO_E_ARG;
    if (c->rec_c_ready && c->rec_c_n && (!out || cap < c->rec_c_n))
        return fail(c, DISCO_E_ARG, "disco_fetch_contained_records: need room for %llu records", (unsigned long long)c->rec_c_n);
    return contained_records_out(c, "disco_fetch_contained_records", out, -1, 0, 16);
}

int disco_write_contained_records(disco_ctx *c, int fd, uint64_t file_offset, uint32_t host_threads)
{
    DISCO_TRACE("disco_write_contained_records");
    if (!c || fd < 0) return DISCO_E_ARG;
    return contained_records_out(c, "disco_write_contained_records", nullptr, fd, file_offset, host_threads);
}

int disco_set_record_piece(disco_ctx *c, uint64_t records)
{
    if (!c) return DISCO_E_ARG;
    c->rec_piece = records;
    return DISCO_OK;
}

/* ---- the overlap graph as GFA 1.0, formatted where the reads, the edges and the keys are (disco_gfa.h) ------------------------------- */
static_assert(GFA_SHORT_MAX == DISCO_SHORT_MAX, "disco_gfa.h reads the long class as the table lays it out");
/* where the pieces of the text go: a RingSink and the file behind it, with pieces of the sizes the lines give them */
struct GfaSink {
    RingSink ring;
    int fd;
    u32 threads;
    u64 cap, unit;    /* bytes a piece may hold; a piece takes the lines that start in one stretch of `unit` bytes (cap - GFA_MAX_LINE) */
    u64 file_off = 0; /* where the next section begins in the file */
    LocalBuf<u64> d_cut;
    GfaSink(disco_ctx *c, const char *who, int fd_, uint64_t piece_bytes, uint32_t host_threads)
        : ring(c, who), fd(fd_), threads(std::max<uint32_t>(host_threads, 1)),
          cap(piece_bytes ? std::min<u64>(std::max<u64>(piece_bytes, 65536), c->ring_half) : c->ring_half), unit(cap - GFA_MAX_LINE), d_cut(c)
    {
    }
    /* the piece just launched into ring.next(), `bytes` long, belongs at byte file_pos of the file */
    int ship(u64 bytes, u64 file_pos) { return ring.ship_piece(bytes, fd, nullptr, file_pos, threads); }
};
/* declared behind a function's LocalBufs, so that it goes before they do: unless the function got to its end (done), it waits for the
 * stream — nothing in flight reads what they release */
struct WaitUnlessDone {
    disco_ctx *c;
    bool done = false;
    ~WaitUnlessDone()
    {
        if (!done) (void)hipStreamSynchronize(c->stream);
    }
};
/* one section of the file — n_lines lines whose starts are place[0 .. n_lines], place[n_lines] = total — piece by piece: launch(a, b,
 * piece) formats the lines [a[0], b[0]) into a piece that begins at byte a[1] of the section (a, b: two entries of gfa_cuts_kernel) */
static int gfa_section(disco_ctx *c, const char *who, GfaSink &o, const u64 *place, u64 n_lines, u64 total, const u32 *ovf, u32 n_long,
                       const std::function<void(const u64 *, const u64 *, char *)> &launch)
{
    if (total == 0) return DISCO_OK;
    const u64 np = (total + o.unit - 1) / o.unit;
    std::vector<u64> cut(3 * (np + 1));
    CHK(ensure(c, o.d_cut, 3 * (np + 1)));
    for (int i = 0; i < 2; i++) CHK(ensure(c, o.ring.piece[i], std::min(o.cap, total))); /* (grow-only; nothing of the section before is in flight) */
    hipLaunchKernelGGL(gfa_cuts_kernel, dim3(flat_grid(c, np + 1)), dim3(256), 0, c->stream, place, n_lines, o.unit, np, ovf, n_long, o.d_cut.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(cut.data(), o.d_cut, cut.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (u64 r = 0; r < np; r++) {
        const u64 *a = &cut[3 * r], *b = &cut[3 * (r + 1)];
        const u64 bytes = b[1] - a[1];
        if (bytes == 0) continue; /* (a line longer than the stretch: the one behind it has no line of its own) */
        if (b[0] < a[0] || b[0] > n_lines || bytes > o.cap) return fail(c, DISCO_E_CAPACITY, "%s: a piece of %llu bytes, room for %llu", who, (unsigned long long)bytes, (unsigned long long)o.cap);
        launch(a, b, (char *)o.ring.next());
        CHK(o.ship(bytes, o.file_off + a[1]));
    }
    o.file_off += total;
    return DISCO_OK;
}
/* a section that is one stream of bytes with no line a piece could end at (the chain S lines of disco_write_gfa_chains: a line can be a
 * genome): piece r is the bytes [r step, (r + 1) step) of it, step = the piece's room rounded down to 16 so that every piece begins
 * 16-byte aligned in the stream as in its buffer; launch(lo, hi, piece) fills the piece with the bytes [lo, hi) */
static int gfa_byte_section(disco_ctx *c, GfaSink &o, u64 total, const std::function<void(u64, u64, char *)> &launch)
{
    if (total == 0) return DISCO_OK;
    const u64 step = o.cap & ~(u64)15;
    for (int i = 0; i < 2; i++) CHK(ensure(c, o.ring.piece[i], std::min(o.cap, total)));
    for (u64 lo = 0; lo < total; lo += step) {
        const u64 hi = std::min(total, lo + step);
        launch(lo, hi, (char *)o.ring.next());
        CHK(o.ship(hi - lo, o.file_off + lo));
    }
    o.file_off += total;
    return DISCO_OK;
}

/* the read table as disco_gfa.h looks at it, whichever of its three layouts it has */
static GfaReads gfa_reads(const disco_ctx *c, const u64 *d_findex)
{
    GfaReads R;
    R.rows = (const uint64_t *)c->d_reads;
    R.S = (u32)c->S;
    R.full = c->two_class ? (const uint64_t *)c->d_full.p : nullptr;
    R.ovf = c->two_class ? c->d_ovf.p : nullptr;
    R.long_ids = c->two_class ? c->d_long_ids.p : nullptr;
    R.SL = c->two_class ? (u32)c->S_ext : 0u;
    R.len = c->d_len;
    R.file_index = (const uint64_t *)d_findex;
    R.n = c->n;
    return R;
}

int64_t disco_write_gfa(disco_ctx *c, int fd, const uint64_t *file_index, uint32_t flags, uint64_t piece_bytes, uint32_t host_threads)
{
    DISCO_TRACE("disco_write_gfa");
    static const char who[] = "disco_write_gfa";
    if (!c || fd < 0) return DISCO_E_ARG;
    if (flags & ~(uint32_t)DISCO_GFA_NO_SEQ) return fail(c, DISCO_E_ARG, "%s: unknown flags %#x", who, flags);
    if (c->comm) return fail(c, DISCO_E_UNSUPPORTED, "%s: a rank holds its share of the graph only", who);
    if (c->phase < 8) return fail(c, DISCO_E_STATE, "%s: run disco_transitive_reduce first", who);
    if (c->n >= (1ull << 31)) return fail(c, DISCO_E_UNSUPPORTED, "%s: more than 2^31 reads", who);
    HIPCHK(c, hipSetDevice(c->device));
    CHK(pinned_ring(c, who));
    const bool no_seq = (flags & DISCO_GFA_NO_SEQ) != 0;
    const u64 n = c->n, ne = c->n_out;
    GfaSink o(c, who, fd, piece_bytes, host_threads);
    LocalBuf<u64> d_findex(c), place(c);
    LocalBuf<u16> sbytes(c), subs(c);
    LocalBuf<u8> bytes(c);
    ContainedGroups G(c);
    WaitUnlessDone settled{c};
    if (file_index) {
        CHK(ensure(c, d_findex, n));
        HIPCHK(c, hipMemcpyAsync(d_findex, file_index, n * 8, hipMemcpyHostToDevice, c->stream));
    }
    static const char header[] = GFA_HEADER;
    if (pwrite(fd, header, sizeof header - 1, 0) != (ssize_t)(sizeof header - 1)) return fail(c, DISCO_E_ARG, "%s: write error", who);
    o.file_off = sizeof header - 1;
    /* S lines: a lane per word of a read */
    const GfaReads R = gfa_reads(c, d_findex);
    u64 total = 0;
    if (n) {
        CHK(ensure(c, sbytes, n));
        CHK(ensure(c, place, n + 1));
        hipLaunchKernelGGL(gfa_s_measure_kernel, dim3(flat_grid(c, n)), dim3(256), 0, c->stream, R, (const u8 *)nullptr, no_seq ? 1u : 0u, sbytes.p);
        CHK((scan_exclusive<u16, u64>(c, sbytes, n, place, true, &total)));
        const u32 W = no_seq ? 1u : R.S;
        const bool long_pass = c->two_class && !no_seq && R.SL > GFA_HEAD_WORDS;
        CHK(gfa_section(c, who, o, place, n, total, R.ovf, (u32)c->n_long, [&](const u64 *a, const u64 *b, char *piece) {
            hipLaunchKernelGGL(gfa_s_write_kernel, dim3(flat_grid(c, (b[0] - a[0]) * W)), dim3(256), 0, c->stream, R, (const u8 *)nullptr, (const u64 *)place, a[0], b[0], a[1], no_seq ? 1u : 0u, W, piece);
            if (long_pass && b[2] > a[2])
                hipLaunchKernelGGL(gfa_s_write_long_kernel, dim3(flat_grid(c, (b[2] - a[2]) * (R.SL - GFA_HEAD_WORDS))), dim3(256), 0, c->stream, R, (const u8 *)nullptr, (const u64 *)place, a[2], b[2],
                                   a[1], piece);
        }));
    }
    /* L lines: a lane per edge, in the order of disco_fetch_edges */
    if (ne) {
        TextView g;
        g.src = c->d_out_src;
        g.ent = c->d_out_ent;
        g.valid = out_valid(c);
        g.pos = out_pos(c);
        g.len = c->d_len;
        g.file_index = d_findex;
        g.n_slots = c->out_used;
        if (c->prm.max_substitutions) { /* by fetch-order rank, as disco_fetch_edge_substitutions has them */
            CHK(ensure(c, subs, ne));
            hipLaunchKernelGGL(edge_subs_kernel, dim3(flat_grid(c, c->out_used)), dim3(256), 0, c->stream, c->d_out_src, c->d_out_ent, out_valid(c), out_pos(c), c->out_used,
                               c->d_reads, c->d_len, c->S, subs.p);
        }
        const u16 *d_subs = c->prm.max_substitutions ? subs.p : nullptr;
        CHK(ensure(c, bytes, ne));
        CHK(ensure(c, place, ne + 1));
        hipLaunchKernelGGL(gfa_l_measure_kernel, dim3(flat_grid(c, g.n_slots)), dim3(256), 0, c->stream, g, d_subs, (const u8 *)nullptr, bytes.p);
        CHK((scan_exclusive<u8, u64>(c, bytes, ne, place, true, &total)));
        const bool dense = c->out_dense;
        CHK(gfa_section(c, who, o, place, ne, total, nullptr, 0, [&](const u64 *a, const u64 *b, char *piece) {
            const u64 s_lo = dense ? a[0] : 0, s_hi = dense ? b[0] : g.n_slots;
            hipLaunchKernelGGL(gfa_l_write_kernel, dim3(flat_grid(c, s_hi - s_lo)), dim3(256), 0, c->stream, g, d_subs, (const u8 *)nullptr, (const u64 *)place, s_lo, s_hi, a[0], b[0], a[1], piece);
        }));
    }
    /* C lines: a lane per contained row, grouped and sorted as for the contained-read files */
    u64 nc = c->n_contained;
    if (nc) {
        CHK(settle_keys(c));
        CHK(group_contained_rows(c, (const u8 *)c->d_contained, 0, n, &nc, G));
        u32 h_ctr[CGRP_CTRS] = {0, 0, 0, 0};
        HIPCHK(c, hipMemcpyAsync(h_ctr, G.ctr, sizeof h_ctr, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (h_ctr[CGRP_BAD_KEYS]) return fail(c, DISCO_E_STATE, "%s: %u contained reads have a key that names no containing read", who, h_ctr[CGRP_BAD_KEYS]);
        CTextView g;
        g.word = G.word;
        g.sup = G.sup;
        g.len = c->d_len;
        g.file_index = d_findex;
        g.nc = nc;
        g.k = (u32)c->k;
        CHK(ensure(c, bytes, nc));
        CHK(ensure(c, place, nc + 1));
        hipLaunchKernelGGL(gfa_c_measure_kernel, dim3(flat_grid(c, nc)), dim3(256), 0, c->stream, g, bytes.p);
        CHK((scan_exclusive<u8, u64>(c, bytes, nc, place, true, &total)));
        CHK(gfa_section(c, who, o, place, nc, total, nullptr, 0, [&](const u64 *a, const u64 *b, char *piece) {
            hipLaunchKernelGGL(gfa_c_write_kernel, dim3(flat_grid(c, b[0] - a[0])), dim3(256), 0, c->stream, g, (const u64 *)place, a[0], b[0], a[1], piece);
        }));
    }
    CHK(o.ring.flush());
    settled.done = true;
    return (int64_t)o.file_off;
}

/* ---- the compacted graph as GFA 1.0: the composite edges of the contraction as segments with their merged bases (disco_gfa_chains.h) ---- */
/* what disco_write_gfa_chains and disco_write_unitig_reads ask before they touch anything */
static int gfu_preconditions(disco_ctx *c, const char *who)
{
    if (c->comm) return fail(c, DISCO_E_UNSUPPORTED, "%s: a rank holds its share of the graph only", who);
    if (c->prm.max_substitutions) return fail(c, DISCO_E_UNSUPPORTED, "%s: with max_substitutions > 0 the reads of a chain disagree about its bases", who);
    if (c->phase < 8) return fail(c, DISCO_E_STATE, "%s: run disco_transitive_reduce first", who);
    if (!c->ch_ready || !c->ch_resident || c->ch_edges_n != c->n_out)
        return fail(c, DISCO_E_STATE, "%s: run disco_contract_chains on the resident edges first (after disco_contract_chains_of the host holds them)", who);
    if (c->n >= (1ull << 31)) return fail(c, DISCO_E_UNSUPPORTED, "%s: more than 2^31 reads", who);
    return DISCO_OK;
}
/* the resident contraction as disco_gfa_chains.h looks at it (lsum: gfu_link_sums) */
static GfuChains gfu_chains(const disco_ctx *c, bool no_seq)
{
    GfuChains H;
    H.comp = (const disco_chain_edge *)c->d_ch_comp.p;
    H.links = (const disco_chain_link *)c->d_ch_links.p;
    H.lsum = H.cplace = nullptr;
    H.n_comp = c->ch_comp_n;
    H.no_seq = no_seq;
    return H;
}
/* skip[i] = 1 for the reads without a segment of their own: the contained ones and the interior reads of the chains */
static int gfu_skip_flags(disco_ctx *c, const GfuChains &H, LocalBuf<u8> &skip)
{
    const u64 n = c->n, nl = c->ch_links_n;
    CHK(ensure(c, skip, n));
    HIPCHK(c, hipMemcpyAsync(skip, c->d_contained, n, hipMemcpyDeviceToDevice, c->stream));
    if (H.n_comp) {
        hipLaunchKernelGGL(gfu_mark_links_kernel, dim3(flat_grid(c, nl)), dim3(256), 0, c->stream, H.links, nl, skip.p);
        hipLaunchKernelGGL(gfu_unmark_ends_kernel, dim3(flat_grid(c, H.n_comp)), dim3(256), 0, c->stream, H.comp, H.n_comp, (const u8 *)c->d_contained, skip.p);
    }
    return DISCO_OK;
}
/* H.lsum: the exclusive scan of the links' offsets, total included (loff: room for the offsets themselves) */
static int gfu_link_sums(disco_ctx *c, GfuChains &H, LocalBuf<u32> &loff, LocalBuf<u64> &lsum)
{
    const u64 nl = c->ch_links_n;
    CHK(ensure(c, loff, nl));
    CHK(ensure(c, lsum, nl + 1));
    hipLaunchKernelGGL(gfu_link_offsets_kernel, dim3(flat_grid(c, nl)), dim3(256), 0, c->stream, H.links, nl, loff.p);
    CHK((scan_exclusive<u32, u64>(c, loff, nl, lsum, true, nullptr)));
    H.lsum = (const uint64_t *)lsum.p;
    return DISCO_OK;
}

int64_t disco_write_gfa_chains(disco_ctx *c, int fd, const uint64_t *file_index, uint32_t flags, uint64_t piece_bytes, uint32_t host_threads)
{
    DISCO_TRACE("disco_write_gfa_chains");
    static const char who[] = "disco_write_gfa_chains";
    if (!c || fd < 0) return DISCO_E_ARG;
    if (flags & ~(uint32_t)DISCO_GFA_NO_SEQ) return fail(c, DISCO_E_ARG, "%s: unknown flags %#x", who, flags);
    CHK(gfu_preconditions(c, who));
    HIPCHK(c, hipSetDevice(c->device));
    CHK(pinned_ring(c, who));
    const bool no_seq = (flags & DISCO_GFA_NO_SEQ) != 0;
    const u64 n = c->n, ne = c->n_out, nk = c->ch_comp_n;
    GfaSink o(c, who, fd, piece_bytes, host_threads);
    LocalBuf<u64> d_findex(c), place(c), lsum(c), cbytes(c), cplace(c);
    LocalBuf<u32> loff(c);
    LocalBuf<u16> sbytes(c);
    LocalBuf<u8> bytes(c), skip(c);
    WaitUnlessDone settled{c};
    if (file_index) {
        CHK(ensure(c, d_findex, n));
        HIPCHK(c, hipMemcpyAsync(d_findex, file_index, n * 8, hipMemcpyHostToDevice, c->stream));
    }
    static const char header[] = GFA_HEADER;
    if (pwrite(fd, header, sizeof header - 1, 0) != (ssize_t)(sizeof header - 1)) return fail(c, DISCO_E_ARG, "%s: write error", who);
    o.file_off = sizeof header - 1;
    const GfaReads R = gfa_reads(c, d_findex);
    GfuChains H = gfu_chains(c, no_seq);
    u64 total = 0;
    /* S lines of the reads that are neither contained nor inside a chain: disco_write_gfa's writers behind the skip flags */
    if (n) {
        CHK(gfu_skip_flags(c, H, skip));
        CHK(ensure(c, sbytes, n));
        CHK(ensure(c, place, n + 1));
        hipLaunchKernelGGL(gfa_s_measure_kernel, dim3(flat_grid(c, n)), dim3(256), 0, c->stream, R, (const u8 *)skip, no_seq ? 1u : 0u, sbytes.p);
        CHK((scan_exclusive<u16, u64>(c, sbytes, n, place, true, &total)));
        const u32 W = no_seq ? 1u : R.S;
        const bool long_pass = c->two_class && !no_seq && R.SL > GFA_HEAD_WORDS;
        CHK(gfa_section(c, who, o, place, n, total, R.ovf, (u32)c->n_long, [&](const u64 *a, const u64 *b, char *piece) {
            hipLaunchKernelGGL(gfa_s_write_kernel, dim3(flat_grid(c, (b[0] - a[0]) * W)), dim3(256), 0, c->stream, R, (const u8 *)skip, (const u64 *)place, a[0], b[0], a[1],
                               no_seq ? 1u : 0u, W, piece);
            if (long_pass && b[2] > a[2])
                hipLaunchKernelGGL(gfa_s_write_long_kernel, dim3(flat_grid(c, (b[2] - a[2]) * (R.SL - GFA_HEAD_WORDS))), dim3(256), 0, c->stream, R, (const u8 *)skip,
                                   (const u64 *)place, a[2], b[2], a[1], piece);
        }));
    }
    /* S lines of the composite edges: one stream of bytes, a lane per 16 of them */
    if (nk) {
        CHK(ensure(c, cbytes, nk));
        CHK(ensure(c, cplace, nk + 1));
        CHK(gfu_link_sums(c, H, loff, lsum));
        hipLaunchKernelGGL(gfu_s_measure_kernel, dim3(flat_grid(c, nk)), dim3(256), 0, c->stream, H, (const u16 *)c->d_len, cbytes.p);
        CHK((scan_exclusive<u64, u64>(c, cbytes, nk, cplace, true, &total)));
        H.cplace = (const uint64_t *)cplace.p;
        CHK(gfa_byte_section(c, o, total, [&](u64 lo, u64 hi, char *piece) {
            hipLaunchKernelGGL(gfu_spell_kernel, dim3(flat_grid(c, gfu_items(lo, hi))), dim3(256), 0, c->stream, R, H, lo, hi, piece);
        }));
    }
    /* L lines of the edges that went into no composite edge, in the order of disco_fetch_edges */
    if (ne) {
        TextView g;
        g.src = c->d_out_src;
        g.ent = c->d_out_ent;
        g.valid = out_valid(c);
        g.pos = out_pos(c);
        g.len = c->d_len;
        g.file_index = d_findex;
        g.n_slots = c->out_used;
        const u8 *dead = c->d_ch_dead;
        CHK(ensure(c, bytes, ne));
        CHK(ensure(c, place, ne + 1));
        hipLaunchKernelGGL(gfa_l_measure_kernel, dim3(flat_grid(c, g.n_slots)), dim3(256), 0, c->stream, g, (const u16 *)nullptr, dead, bytes.p);
        CHK((scan_exclusive<u8, u64>(c, bytes, ne, place, true, &total)));
        const bool dense = c->out_dense;
        CHK(gfa_section(c, who, o, place, ne, total, nullptr, 0, [&](const u64 *a, const u64 *b, char *piece) {
            const u64 s_lo = dense ? a[0] : 0, s_hi = dense ? b[0] : g.n_slots;
            hipLaunchKernelGGL(gfa_l_write_kernel, dim3(flat_grid(c, s_hi - s_lo)), dim3(256), 0, c->stream, g, (const u16 *)nullptr, dead, (const u64 *)place, s_lo, s_hi, a[0], b[0],
                               a[1], piece);
        }));
    }
    /* ... and the head and the tail link of every composite edge, a lane per composite edge */
    if (nk) {
        CHK(ensure(c, bytes, nk));
        CHK(ensure(c, place, nk + 1));
        hipLaunchKernelGGL(gfu_l_measure_kernel, dim3(flat_grid(c, nk)), dim3(256), 0, c->stream, R, H, bytes.p);
        CHK((scan_exclusive<u8, u64>(c, bytes, nk, place, true, &total)));
        CHK(gfa_section(c, who, o, place, nk, total, nullptr, 0, [&](const u64 *a, const u64 *b, char *piece) {
            hipLaunchKernelGGL(gfu_l_write_kernel, dim3(flat_grid(c, b[0] - a[0])), dim3(256), 0, c->stream, R, H, (const u64 *)place, a[0], b[0], a[1], piece);
        }));
    }
    CHK(o.ring.flush());
    settled.done = true;
    return (int64_t)o.file_off;
}

/* ---- every read placed on its segment of the compacted graph, and every segment's reads and bases (disco_unitig_reads.h) -------------- */
int64_t disco_write_unitig_reads(disco_ctx *c, int fd, const uint64_t *file_index, uint32_t flags, uint64_t piece_bytes, uint32_t host_threads)
{
    DISCO_TRACE("disco_write_unitig_reads");
    static const char who[] = "disco_write_unitig_reads";
    if (!c || fd < 0) return DISCO_E_ARG;
    if (flags & ~(uint32_t)DISCO_UNITIG_READS_DEPTH_ONLY) return fail(c, DISCO_E_ARG, "%s: unknown flags %#x", who, flags);
    CHK(gfu_preconditions(c, who));
    HIPCHK(c, hipSetDevice(c->device));
    CHK(pinned_ring(c, who));
    const bool depth_only = (flags & DISCO_UNITIG_READS_DEPTH_ONLY) != 0, verbose = getenv("DISCO_VERBOSE") != nullptr;
    const u64 n = c->n, nk = c->ch_comp_n, nl = c->ch_links_n;
    const auto t0 = std::chrono::steady_clock::now();
    GfaSink o(c, who, fd, piece_bytes, host_threads);
    LocalBuf<u64> d_findex(c), place(c), lsum(c), st_a(c), st_b(c), cpos(c), rbases(c), lbases(c), kcnt(c), kbases(c);
    LocalBuf<u32> loff(c), cseg(c), rcnt(c), lcnt(c), flag(c);
    LocalBuf<u8> bytes(c), skip(c);
    WaitUnlessDone settled{c};
    if (file_index) {
        CHK(ensure(c, d_findex, n));
        HIPCHK(c, hipMemcpyAsync(d_findex, file_index, n * 8, hipMemcpyHostToDevice, c->stream));
    }
    const GfaReads R = gfa_reads(c, d_findex);
    GfuChains H = gfu_chains(c, false);
    UtrView V;
    V.state = V.cpos = V.rbases = V.kcnt = V.kbases = nullptr;
    V.cseg = V.rcnt = nullptr;
    u32 rounds = 0;
    if (n) {
        /* roots: the initial states, then rounds of doubling until one moves nobody. flag[0]: keys that name no read; flag[1 + r]: round r moved somebody */
        CHK(settle_keys(c));
        CHK(ensure(c, st_a, n));
        CHK(ensure(c, st_b, n));
        CHK(ensure(c, flag, 1 + UTR_MAX_ROUNDS));
        HIPCHK(c, hipMemsetAsync(flag, 0, (1 + UTR_MAX_ROUNDS) * sizeof(u32), c->stream));
        hipLaunchKernelGGL(utr_init_kernel, dim3(flat_grid(c, n)), dim3(256), 0, c->stream, (const u64 *)c->d_best, (const u8 *)c->d_contained, (const u16 *)c->d_len, n, (u32)c->k, (uint64_t *)st_a.p, flag.p);
        HIPCHK(c, hipGetLastError());
        u32 h_flag = 0;
        HIPCHK(c, hipMemcpyAsync(&h_flag, flag, sizeof h_flag, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (h_flag) return fail(c, DISCO_E_STATE, "%s: %u contained reads have a key that names no containing read", who, h_flag);
        uint64_t *cur = (uint64_t *)st_a.p, *next = (uint64_t *)st_b.p;
        bool moving = c->n_contained != 0;
        while (moving && rounds < UTR_MAX_ROUNDS) {
            hipLaunchKernelGGL(utr_round_kernel, dim3(flat_grid(c, n)), dim3(256), 0, c->stream, (const uint64_t *)cur, next, (const u16 *)c->d_len, n, flag.p + 1 + rounds);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(&h_flag, flag.p + 1 + rounds, sizeof h_flag, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            std::swap(cur, next);
            moving = h_flag != 0;
            rounds++;
        }
        if (moving) return fail(c, DISCO_E_STATE, "%s: the containment keys do not settle in %u rounds of doubling: they hold a cycle", who, UTR_MAX_ROUNDS);
        V.state = (const uint64_t *)cur;
        /* segments: the interior reads of the chains at their s_j; everybody else is a segment of their own */
        CHK(ensure(c, cseg, n));
        CHK(ensure(c, cpos, n));
        HIPCHK(c, hipMemsetAsync(cseg, 0xFF, n * sizeof(u32), c->stream));
        if (nk) {
            CHK(gfu_link_sums(c, H, loff, lsum));
            hipLaunchKernelGGL(utr_place_links_kernel, dim3(flat_grid(c, nl)), dim3(256), 0, c->stream, H, nl, cseg.p, (uint64_t *)cpos.p);
        }
        V.cseg = cseg.p;
        V.cpos = (const uint64_t *)cpos.p;
        /* counts: every read to its root, then the chains' totals as differences of one scan in link order */
        CHK(ensure(c, rcnt, n));
        CHK(ensure(c, rbases, n));
        HIPCHK(c, hipMemsetAsync(rcnt, 0, n * sizeof(u32), c->stream));
        HIPCHK(c, hipMemsetAsync(rbases, 0, n * sizeof(u64), c->stream));
        hipLaunchKernelGGL(utr_count_kernel, dim3(flat_grid(c, n)), dim3(256), 0, c->stream, V.state, (const u16 *)c->d_len, n, rcnt.p, rbases.p);
        V.rcnt = rcnt.p;
        V.rbases = (const uint64_t *)rbases.p;
        if (nk) {
            CHK(ensure(c, lcnt, nl));
            CHK(ensure(c, lbases, nl));
            CHK(ensure(c, kcnt, nl + 1));
            CHK(ensure(c, kbases, nl + 1));
            hipLaunchKernelGGL(utr_gather_kernel, dim3(flat_grid(c, nl)), dim3(256), 0, c->stream, H, nl, (const u32 *)rcnt, (const u64 *)rbases, lcnt.p, lbases.p);
            CHK((scan_exclusive<u32, u64>(c, lcnt, nl, kcnt, true, nullptr)));
            CHK((scan_exclusive<u64, u64>(c, lbases, nl, kbases, true, nullptr)));
            V.kcnt = (const uint64_t *)kcnt.p;
            V.kbases = (const uint64_t *)kbases.p;
        }
        HIPCHK(c, hipGetLastError());
    }
    double ms_resolve = 0;
    if (verbose) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        ms_resolve = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    static const char header[] = UTR_HEADER;
    if (pwrite(fd, header, sizeof header - 1, 0) != (ssize_t)(sizeof header - 1)) return fail(c, DISCO_E_ARG, "%s: write error", who);
    o.file_off = sizeof header - 1;
    u64 total = 0;
    /* U lines of the read segments: a lane per read behind the skip flags of the S lines */
    if (n) {
        CHK(gfu_skip_flags(c, H, skip));
        CHK(ensure(c, bytes, n));
        CHK(ensure(c, place, n + 1));
        hipLaunchKernelGGL(utr_u_read_measure_kernel, dim3(flat_grid(c, n)), dim3(256), 0, c->stream, R, V, (const u8 *)skip, bytes.p);
        CHK((scan_exclusive<u8, u64>(c, bytes, n, place, true, &total)));
        CHK(gfa_section(c, who, o, place, n, total, nullptr, 0, [&](const u64 *a, const u64 *b, char *piece) {
            hipLaunchKernelGGL(utr_u_read_write_kernel, dim3(flat_grid(c, b[0] - a[0])), dim3(256), 0, c->stream, R, V, (const u8 *)skip, (const u64 *)place, a[0], b[0], a[1], piece);
        }));
    }
    /* U lines of the composite edges: a lane per composite edge */
    if (nk) {
        CHK(ensure(c, bytes, nk));
        CHK(ensure(c, place, nk + 1));
        hipLaunchKernelGGL(utr_u_chain_measure_kernel, dim3(flat_grid(c, nk)), dim3(256), 0, c->stream, R, H, V, bytes.p);
        CHK((scan_exclusive<u8, u64>(c, bytes, nk, place, true, &total)));
        CHK(gfa_section(c, who, o, place, nk, total, nullptr, 0, [&](const u64 *a, const u64 *b, char *piece) {
            hipLaunchKernelGGL(utr_u_chain_write_kernel, dim3(flat_grid(c, b[0] - a[0])), dim3(256), 0, c->stream, R, H, V, (const u64 *)place, a[0], b[0], a[1], piece);
        }));
    }
    /* R lines: a lane per read */
    if (n && !depth_only) {
        CHK(ensure(c, bytes, n));
        CHK(ensure(c, place, n + 1));
        hipLaunchKernelGGL(utr_r_measure_kernel, dim3(flat_grid(c, n)), dim3(256), 0, c->stream, R, V, bytes.p);
        CHK((scan_exclusive<u8, u64>(c, bytes, n, place, true, &total)));
        CHK(gfa_section(c, who, o, place, n, total, nullptr, 0, [&](const u64 *a, const u64 *b, char *piece) {
            hipLaunchKernelGGL(utr_r_write_kernel, dim3(flat_grid(c, b[0] - a[0])), dim3(256), 0, c->stream, R, V, (const u64 *)place, a[0], b[0], a[1], piece);
        }));
    }
    CHK(o.ring.flush());
    settled.done = true;
    if (verbose)
        fprintf(stderr, "[disco] unitig reads: %u rounds of doubling moved a read; roots, places and counts in %.3f ms; %llu bytes in %.3f ms\n", rounds ? rounds - 1 : 0u, ms_resolve, (unsigned long long)o.file_off,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    return (int64_t)o.file_off;
}

/* the contained rows of the current flags start their way to the host now, on a side stream (grouped: also in the order of the
 * contained-read files), instead of when they are asked for: for callers that have work between disco_mark_contained and
 * disco_fetch_contained[_grouped] — buildG: edge selection and the reduction (they lose 1-3 ms to the side stream; the fetch then
 * only waits for what is left and decodes) */
int disco_start_contained_rows(disco_ctx *c, int grouped)
{
    if (!c) return DISCO_E_ARG;
    if (c->phase < 4) return fail(c, DISCO_E_STATE, "disco_start_contained_rows: run disco_mark_contained first");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->n_contained == 0) return DISCO_OK;
    return start_contained_rows(c, grouped != 0);
}

/* ---- chains of the reduced graph as composite edges (kernels and the argument: disco_chains.h) ------------- */
static int contract_chains(disco_ctx *c, const u64 *d_src, const u64 *d_ent, const u8 *d_valid, const u64 *d_pos, u64 n_slots, u64 ne, u64 n, u32 min_ovl)
{
    DISCO_TRACE("contract_chains");
    c->ch_ready = false;
    c->ptext.bytes = 0; /* (a text formatted from the contraction before this one names composite edges that are gone) */
    c->ptext.off.clear();
    if (n_slots >= (1ull << 31)) return fail(c, DISCO_E_UNSUPPORTED, "chain contraction: more than 2^31 edge slots");
    ChainView g;
    g.src = d_src;
    g.ent = d_ent;
    g.valid = d_valid;
    g.pos = d_pos;
    g.len = c->d_len;
    g.n_slots = n_slots;
    g.min_ovl = min_ovl;
    LocalBuf<u32> deg(c), he(c), links_of(c), live(c);
    LocalBuf<u8> internal(c), is_head(c);
    LocalBuf<ChRank> ra(c), rb(c);
    LocalBuf<u64> comp_id(c), link_start(c);
    const u64 n_half = 2 * n_slots;
    CHK(ensure(c, deg, n));
    CHK(ensure(c, he, 2 * n));
    CHK(ensure(c, internal, n));
    CHK(ensure(c, ra, n_half));
    CHK(ensure(c, rb, n_half));
    CHK(ensure(c, live, 1));
    HIPCHK(c, hipMemsetAsync(deg, 0, n * sizeof(u32), c->stream));
    hipLaunchKernelGGL(ch_degree_kernel, dim3(flat_grid(c, n_slots)), dim3(256), 0, c->stream, g, deg, he);
    hipLaunchKernelGGL(ch_internal_kernel, dim3(flat_grid(c, n)), dim3(256), 0, c->stream, g, deg, he, n, internal);
    hipLaunchKernelGGL(ch_init_kernel, dim3(flat_grid(c, n_slots)), dim3(256), 0, c->stream, g, internal, he, ra);
    HIPCHK(c, hipGetLastError());
    /* a chain of L half-edges is ranked after ceil(log2 L) rounds and no chain has more than n_half elements; a ring of
     * absorbable nodes never finishes (its elements are discarded by ch_heads_kernel and left to the host pass), so the
     * rounds stop at that bound instead of running while anything is live */
    int max_rounds = 1;
    while (max_rounds < 32 && (1ull << max_rounds) < n_half) ++max_rounds;
    for (int round = 0; round < max_rounds; round++) {
        u32 h_live = 0;
        HIPCHK(c, hipMemsetAsync(live, 0, sizeof(u32), c->stream));
        hipLaunchKernelGGL(ch_jump_kernel, dim3(flat_grid(c, n_half)), dim3(256), 0, c->stream, ra, rb, n_half, live);
        HIPCHK(c, hipMemcpyAsync(&h_live, live, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        std::swap<DevBuf<ChRank>>(ra, rb); /* (the memory changes hands; both stay the function's) */
        if (!h_live) break;
    }
    release(c, rb); /* (the ranking is done: not held while the composite edges are emitted) */
    release(c, deg);
    CHK(ensure(c, is_head, n_slots));
    CHK(ensure(c, links_of, n_slots));
    CHK(ensure(c, c->d_ch_dead, std::max<u64>(ne, 1)));
    HIPCHK(c, hipMemsetAsync(c->d_ch_dead, 0, std::max<u64>(ne, 1), c->stream));
    hipLaunchKernelGGL(ch_heads_kernel, dim3(flat_grid(c, n_slots)), dim3(256), 0, c->stream, g, internal, ra, is_head, links_of, c->d_ch_dead);
    CHK(ensure(c, comp_id, n_slots + 1));
    CHK(ensure(c, link_start, n_slots + 1));
    u64 n_comp = 0, n_links = 0;
    CHK((scan_exclusive<u8, u64>(c, is_head, n_slots, comp_id, false, &n_comp)));
    CHK((scan_exclusive<u32, u64>(c, links_of, n_slots, link_start, false, &n_links)));
    CHK(ensure(c, c->d_ch_comp, std::max<u64>(n_comp, 1)));
    CHK(ensure(c, c->d_ch_links, std::max<u64>(n_links, 1)));
    CHK(ensure(c, c->d_ch_first, std::max<u64>(n_comp, 1)));
    hipLaunchKernelGGL(ch_emit_kernel, dim3(flat_grid(c, n_slots)), dim3(256), 0, c->stream, g, internal, ra, comp_id, link_start, c->d_ch_comp, c->d_ch_links,
                       c->d_ch_first);
    HIPCHK(c, hipGetLastError());
    /* the residue, compacted in fetch order (the flags and the scan reuse the buffers of the heads, which the emission is through with) */
    u64 n_res = 0;
    hipLaunchKernelGGL(ch_residue_flag_kernel, dim3(flat_grid(c, n_slots)), dim3(256), 0, c->stream, g, (const u8 *)c->d_ch_dead, is_head.p);
    CHK((scan_exclusive<u8, u64>(c, is_head, n_slots, comp_id, false, &n_res)));
    CHK(ensure(c, c->d_ch_res_pos, std::max<u64>(n_res, 1)));
    CHK(ensure(c, c->d_ch_res_slot, std::max<u64>(n_res, 1)));
    hipLaunchKernelGGL(ch_residue_scatter_kernel, dim3(flat_grid(c, n_slots)), dim3(256), 0, c->stream, g, (const u8 *)is_head, (const u64 *)comp_id, c->d_ch_res_pos.p,
                       c->d_ch_res_slot.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->ch_res_n = n_res;
    c->ch_comp_n = n_comp;
    c->ch_links_n = n_links;
    c->ch_edges_n = ne;
    c->ch_ready = true;
    return DISCO_OK;
}

int disco_contract_chains(disco_ctx *c, uint32_t min_overlap_simplify, uint64_t *n_composite, uint64_t *n_links)
{
    if (!c) return DISCO_E_ARG;
    if (c->phase < 8) return fail(c, DISCO_E_STATE, "disco_contract_chains: run disco_transitive_reduce first");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->n_out == 0) {
        c->ch_comp_n = c->ch_links_n = c->ch_edges_n = c->ch_res_n = 0;
        c->ch_ready = true;
    } else
        CHK(contract_chains(c, c->d_out_src, c->d_out_ent, out_valid(c), out_pos(c), c->out_used, c->n_out, c->n, min_overlap_simplify));
    c->ch_resident = true;
    if (n_composite) *n_composite = c->ch_comp_n;
    if (n_links) *n_links = c->ch_links_n;
    return DISCO_OK;
}

int disco_contract_chains_of(disco_ctx *c, const disco_edge *edges, uint64_t n_edges, uint32_t min_overlap_simplify, uint64_t *n_composite, uint64_t *n_links)
{
    if (!c || (n_edges && !edges)) return DISCO_E_ARG;
    if (c->phase < 1) return fail(c, DISCO_E_STATE, "disco_contract_chains_of: the context holds no reads (their lengths are needed)");
    HIPCHK(c, hipSetDevice(c->device));
    c->ch_ready = false;
    c->ch_resident = false;
    if (n_edges == 0) {
        c->ch_comp_n = c->ch_links_n = c->ch_edges_n = c->ch_res_n = 0;
        c->ch_ready = true;
    } else {
        LocalBuf<u64> d_src(c), d_ent(c), d_pos(c);
        LocalBuf<u8> d_valid(c);
        std::unique_ptr<u64[]> hs(new u64[n_edges]), he(new u64[n_edges]);
        std::atomic<bool> bad{false};
        parallel_for(n_edges, [&](u64 b, u64 e_) {
            for (u64 i = b; i < e_; i++) {
                if (edges[i].src >= c->n || edges[i].dst >= c->n) bad.store(true, std::memory_order_relaxed);
                hs[i] = edges[i].src;
                he[i] = ADJ_MAKE(edges[i].offset, edges[i].dst, edges[i].orient, edges[i].len_dst);
            }
        });
        if (bad) return fail(c, DISCO_E_ARG, "disco_contract_chains_of: an edge names a read the context does not hold");
        CHK(ensure(c, d_src, n_edges));
        CHK(ensure(c, d_ent, n_edges));
        CHK(ensure(c, d_pos, n_edges));
        CHK(ensure(c, d_valid, n_edges));
        if (hipMemcpyAsync(d_src, hs.get(), n_edges * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            hipMemcpyAsync(d_ent, he.get(), n_edges * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess || hipMemsetAsync(d_valid, 1, n_edges, c->stream) != hipSuccess)
            return fail(c, DISCO_E_HIP, "disco_contract_chains_of: upload failed");
        hipLaunchKernelGGL(iota_u64_kernel, dim3(flat_grid(c, n_edges)), dim3(256), 0, c->stream, d_pos, n_edges);
        CHK(contract_chains(c, d_src, d_ent, d_valid, d_pos, n_edges, n_edges, c->n, min_overlap_simplify));
    }
    if (n_composite) *n_composite = c->ch_comp_n;
    if (n_links) *n_links = c->ch_links_n;
    return DISCO_OK;
}

int disco_fetch_chains(disco_ctx *c, disco_chain_edge *comp, disco_chain_link *links, uint8_t *edge_absorbed)
{
    if (!c) return DISCO_E_ARG;
    if (!c->ch_ready) return fail(c, DISCO_E_STATE, "disco_fetch_chains: run disco_contract_chains first");
    HIPCHK(c, hipSetDevice(c->device));
    static_assert(sizeof(disco_chain_edge) == sizeof(ChainEdgeOut) && sizeof(disco_chain_link) == sizeof(ChainLinkOut), "chain records");
    if (comp && c->ch_comp_n) HIPCHK(c, hipMemcpyAsync(comp, c->d_ch_comp, c->ch_comp_n * sizeof(ChainEdgeOut), hipMemcpyDeviceToHost, c->stream));
    if (links && c->ch_links_n) HIPCHK(c, hipMemcpyAsync(links, c->d_ch_links, c->ch_links_n * sizeof(ChainLinkOut), hipMemcpyDeviceToHost, c->stream));
    if (edge_absorbed && c->ch_edges_n) HIPCHK(c, hipMemcpyAsync(edge_absorbed, c->d_ch_dead, c->ch_edges_n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DISCO_OK;
}

int64_t disco_fetch_chain_residue(disco_ctx *c, uint64_t *edge_index, disco_edge *edges, uint64_t cap)
{
    if (!c) return DISCO_E_ARG;
    if (!c->ch_ready) return fail(c, DISCO_E_STATE, "disco_fetch_chain_residue: run disco_contract_chains first");
    const u64 nr = c->ch_res_n;
    if (!edge_index && !edges) return (int64_t)nr;
    if (edges && !c->ch_resident) return fail(c, DISCO_E_STATE, "disco_fetch_chain_residue: the edges were the caller's (disco_contract_chains_of): it holds the records");
    if (cap < nr) return fail(c, DISCO_E_ARG, "disco_fetch_chain_residue: need room for %llu edges", (unsigned long long)nr);
    if (nr == 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    static_assert(sizeof(disco_edge) == sizeof(ChEdgeOut) && sizeof(uint64_t) == sizeof(u64), "residue records");
    LocalBuf<ChEdgeOut> rec(c);
    if (edge_index) HIPCHK(c, hipMemcpyAsync(edge_index, c->d_ch_res_pos, nr * 8, hipMemcpyDeviceToHost, c->stream));
    if (edges) {
        CHK(ensure(c, rec, nr));
        hipLaunchKernelGGL(ch_residue_records_kernel, dim3(flat_grid(c, nr)), dim3(256), 0, c->stream, (const u64 *)c->d_out_src, (const u64 *)c->d_out_ent, (const u16 *)c->d_len,
                           (const u64 *)c->d_ch_res_slot, nr, rec.p);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(edges, rec, nr * sizeof(ChEdgeOut), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return (int64_t)nr;
}

int disco_fetch_chain_first_edges(disco_ctx *c, uint64_t *first_edge)
{
    if (!c || (!first_edge && c->ch_ready && c->ch_comp_n)) return DISCO_E_ARG;
    if (!c->ch_ready) return fail(c, DISCO_E_STATE, "disco_fetch_chain_first_edges: run disco_contract_chains first");
    if (c->ch_comp_n == 0) return DISCO_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(first_edge, c->d_ch_first, c->ch_comp_n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DISCO_OK;
}

int disco_fetch_chain_end_links(disco_ctx *c, disco_chain_link *first, disco_chain_link *last_reversed)
{
    if (!c || ((!first || !last_reversed) && c->ch_ready && c->ch_comp_n)) return DISCO_E_ARG;
    if (!c->ch_ready) return fail(c, DISCO_E_STATE, "disco_fetch_chain_end_links: run disco_contract_chains first");
    const u64 nc = c->ch_comp_n;
    if (nc == 0) return DISCO_OK;
    HIPCHK(c, hipSetDevice(c->device));
    LocalBuf<ChainLinkOut> d(c);
    CHK(ensure(c, d, 2 * nc));
    hipLaunchKernelGGL(ch_end_links_kernel, dim3(flat_grid(c, nc)), dim3(256), 0, c->stream, (const ChainEdgeOut *)c->d_ch_comp, (const ChainLinkOut *)c->d_ch_links,
                       (const u16 *)c->d_len, nc, d.p, d.p + nc);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(first, d.p, nc * sizeof(ChainLinkOut), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(last_reversed, d.p + nc, nc * sizeof(ChainLinkOut), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DISCO_OK;
}

/* ---- the lines of the ParSimpleEdges files from the host pass's description and the device's link arrays (disco_partext.h) ---- */
int64_t disco_format_par_simple(disco_ctx *c, uint32_t n_files, const uint64_t *file_index, const disco_ps_edge *edges, uint64_t n_edges, const disco_ps_piece *pieces,
                                uint64_t n_pieces, uint64_t *file_offsets)
{
    DISCO_TRACE("disco_format_par_simple");
    if (!c || !file_offsets || n_files == 0 || (n_edges && !edges) || (n_pieces && !pieces)) return DISCO_E_ARG;
    if (!c->ch_ready) return fail(c, DISCO_E_STATE, "disco_format_par_simple: run disco_contract_chains first");
    HIPCHK(c, hipSetDevice(c->device));
    for (uint32_t f = 0; f <= n_files; f++) file_offsets[f] = 0;
    c->ptext.bytes = 0;
    c->ptext.off.assign((size_t)n_files + 1, 0);
    if (n_edges == 0) return 0;
    /* the description is small: everything a lane will index with is checked here, before anything is launched */
    std::vector<disco_chain_edge> comp(c->ch_comp_n);
    if (c->ch_comp_n) {
        HIPCHK(c, hipMemcpyAsync(comp.data(), c->d_ch_comp, c->ch_comp_n * sizeof(ChainEdgeOut), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    std::vector<u64> piece_link(n_pieces + 1, 0), edge_item(n_edges + 1, 0), first_item((size_t)n_files + 1, 0);
    for (u64 p = 0; p < n_pieces; p++) {
        const disco_ps_piece &x = pieces[p];
        u64 nl = 1;
        if (x.kind == 0) {
            if (x.a >= c->n) return fail(c, DISCO_E_ARG, "disco_format_par_simple: piece %llu names read %u of %llu", (unsigned long long)p, x.a, (unsigned long long)c->n);
        } else if (x.kind == 1 || x.kind == 2) {
            if (x.a >= c->ch_comp_n)
                return fail(c, DISCO_E_ARG, "disco_format_par_simple: piece %llu names composite edge %u of %llu", (unsigned long long)p, x.a, (unsigned long long)c->ch_comp_n);
            nl = comp[x.a].n_links;
        } else
            return fail(c, DISCO_E_ARG, "disco_format_par_simple: piece %llu is of kind %u", (unsigned long long)p, x.kind);
        piece_link[p + 1] = piece_link[p] + nl;
    }
    uint32_t file = 0;
    for (u64 e = 0; e < n_edges; e++) {
        const disco_ps_edge &x = edges[e];
        if (x.n_pieces == 0 || x.first_piece > n_pieces || x.n_pieces > n_pieces - x.first_piece)
            return fail(c, DISCO_E_ARG, "disco_format_par_simple: the pieces of edge %llu lie outside the %llu given", (unsigned long long)e, (unsigned long long)n_pieces);
        if (x.src >= c->n || x.dst >= c->n) return fail(c, DISCO_E_ARG, "disco_format_par_simple: edge %llu names a read the context does not hold", (unsigned long long)e);
        if (x.file >= n_files || x.file < file) return fail(c, DISCO_E_ARG, "disco_format_par_simple: the files of the edges must ascend and lie below %u (edge %llu)", n_files, (unsigned long long)e);
        edge_item[e + 1] = edge_item[e] + (piece_link[x.first_piece + x.n_pieces] - piece_link[x.first_piece]);
        for (; file < x.file; file++) first_item[(size_t)file + 1] = edge_item[e];
    }
    const u64 n_items = edge_item[n_edges];
    for (; file < n_files; file++) first_item[(size_t)file + 1] = n_items;
    LocalBuf<disco_ps_edge> d_edges(c);
    LocalBuf<disco_ps_piece> d_pieces(c);
    LocalBuf<u64> d_edge_item(c), d_piece_link(c), d_first_item(c), d_findex(c), place(c), d_off(c);
    LocalBuf<u8> bytes(c);
    std::vector<u64> off((size_t)n_files + 1, 0); /* (the context's offsets — all 0 — change only once the text is there) */
    CHK(ensure(c, d_edges, n_edges));
    CHK(ensure(c, d_pieces, std::max<u64>(n_pieces, 1)));
    CHK(ensure(c, d_edge_item, n_edges + 1));
    CHK(ensure(c, d_piece_link, n_pieces + 1));
    CHK(ensure(c, d_first_item, (u64)n_files + 1));
    CHK(ensure(c, d_off, (u64)n_files + 1));
    CHK(ensure(c, bytes, n_items));
    CHK(ensure(c, place, n_items + 1));
    HIPCHK(c, hipMemcpyAsync(d_edges, edges, n_edges * sizeof(disco_ps_edge), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_pieces, pieces, n_pieces * sizeof(disco_ps_piece), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_edge_item, edge_item.data(), (n_edges + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_piece_link, piece_link.data(), (n_pieces + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_first_item, first_item.data(), ((size_t)n_files + 1) * 8, hipMemcpyHostToDevice, c->stream));
    if (file_index) {
        CHK(ensure(c, d_findex, c->n));
        HIPCHK(c, hipMemcpyAsync(d_findex, file_index, c->n * 8, hipMemcpyHostToDevice, c->stream));
    }
    PsView g;
    g.edges = d_edges;
    g.pieces = d_pieces;
    g.edge_item = (const uint64_t *)d_edge_item.p;
    g.piece_link = (const uint64_t *)d_piece_link.p;
    g.comp = (const disco_chain_edge *)c->d_ch_comp.p;
    g.links = (const disco_chain_link *)c->d_ch_links.p;
    g.len = c->d_len;
    g.file_index = (const uint64_t *)d_findex.p;
    g.n_edges = n_edges;
    g.n_pieces = n_pieces;
    g.n_items = n_items;
    hipLaunchKernelGGL(ptext_measure_kernel, dim3(flat_grid(c, n_items)), dim3(256), 0, c->stream, g, bytes.p);
    u64 total = 0;
    CHK((scan_exclusive<u8, u64>(c, bytes, n_items, place, true, &total)));
    hipLaunchKernelGGL(ptext_offsets_kernel, dim3(1), dim3(256), 0, c->stream, (const uint64_t *)d_first_item.p, (const u64 *)place, n_files, (uint64_t *)d_off.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(off.data(), d_off, ((size_t)n_files + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    CHK(ensure(c, c->ptext.d, std::max<u64>(total, 1)));
    hipLaunchKernelGGL(ptext_write_kernel, dim3(flat_grid(c, n_items)), dim3(256), 0, c->stream, g, (const u64 *)place, c->ptext.d.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->ptext.off.swap(off);
    c->ptext.bytes = total;
    for (uint32_t f = 0; f <= n_files; f++) file_offsets[f] = c->ptext.off[f];
    if (getenv("DISCO_VERBOSE"))
        fprintf(stderr, "[disco] par-simple lines: %llu edges, %llu pieces, %llu items, %llu bytes\n", (unsigned long long)n_edges, (unsigned long long)n_pieces,
                (unsigned long long)n_items, (unsigned long long)c->ptext.bytes);
    return (int64_t)c->ptext.bytes;
}

int disco_fetch_par_simple_text(disco_ctx *c, char *out, uint64_t cap) { return c ? fetch_text(c, "disco_fetch_par_simple_text", c->ptext, out, cap) : DISCO_E_ARG; }

int disco_write_par_simple_text(disco_ctx *c, const int *fds, uint32_t n_files, uint32_t)
{
    DISCO_TRACE("disco_write_par_simple_text");
    return c ? write_text(c, "disco_write_par_simple_text", "disco_format_par_simple", c->ptext, fds, n_files) : DISCO_E_ARG;
}

int disco_set_query_order(disco_ctx *c, const void *d_order_u64)
{
    if (!c) return DISCO_E_ARG;
    c->d_order = (const u64 *)d_order_u64;
    c->order_external = d_order_u64 != nullptr;
    return DISCO_OK;
}

int disco_get_query_order(disco_ctx *c, const void **d_order_u64)
{
    if (!c || !d_order_u64) return DISCO_E_ARG;
    *d_order_u64 = c->d_order_used;
    return DISCO_OK;
}

int disco_phase_ms(disco_ctx *c, float *ms, int n)
{
    if (!c || !ms) return DISCO_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    ph_collect(c);
    for (int i = 0; i < n && i < DISCO_PH_COUNT; i++) ms[i] = c->ph_ms[i];
    return DISCO_OK;
}

int disco_memcpy_d2d(disco_ctx *c, void *dst, const void *src, uint64_t bytes)
{
    if (!c || (bytes && (!dst || !src))) return DISCO_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (bytes) HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DISCO_OK;
}

int disco_measure_hbm(disco_ctx *c, uint64_t bytes, int reps, double *gb_per_s)
{
    if (!c || !gb_per_s || bytes < 4096 || reps < 1) return DISCO_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const u64 n = bytes / sizeof(ulonglong2);
    ulonglong2 *src = nullptr, *dst = nullptr;
    if (hipMalloc(&src, n * sizeof(ulonglong2)) != hipSuccess || hipMalloc(&dst, n * sizeof(ulonglong2)) != hipSuccess) {
        if (src) (void)hipFree(src);
        return fail(c, DISCO_E_NOMEM, "disco_measure_hbm: cannot allocate 2 x %llu bytes", (unsigned long long)bytes);
    }
    hipEvent_t e0, e1;
    HIPCHK(c, hipEventCreate(&e0));
    HIPCHK(c, hipEventCreate(&e1));
    HIPCHK(c, hipMemsetAsync(src, 0x5A, n * sizeof(ulonglong2), c->stream));
    const int grid = c->n_cu * 16;
    float best = 1e30f;
    for (int r = 0; r <= reps; r++) { /* launch 0 warms up */
        HIPCHK(c, hipEventRecord(e0, c->stream));
        hipLaunchKernelGGL(stream_copy_kernel, dim3(grid), dim3(256), 0, c->stream, src, dst, n);
        HIPCHK(c, hipEventRecord(e1, c->stream));
        HIPCHK(c, hipEventSynchronize(e1));
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, e0, e1));
        if (r > 0 && ms < best) best = ms;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipFree(src);
    (void)hipFree(dst);
    *gb_per_s = 2.0 * (double)(n * sizeof(ulonglong2)) / ((double)best * 1e-3) / 1e9;
    return DISCO_OK;
}

int disco_measure_gather(disco_ctx *c, uint64_t bytes, int reps, double *gb_per_s)
{
    if (!c || !gb_per_s || bytes < 4096 || reps < 1) return DISCO_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const u64 nrows = bytes / 64;
    ulonglong2 *tab = nullptr;
    u64 *sink = nullptr;
    if (hipMalloc(&tab, nrows * 64) != hipSuccess) return fail(c, DISCO_E_NOMEM, "disco_measure_gather: cannot allocate %llu bytes", (unsigned long long)bytes);
    HIPCHK(c, hipMalloc(&sink, 64));
    hipEvent_t e0, e1;
    HIPCHK(c, hipEventCreate(&e0));
    HIPCHK(c, hipEventCreate(&e1));
    HIPCHK(c, hipMemsetAsync(tab, 0x5A, nrows * 64, c->stream));
    const int grid = c->n_cu * 64; /* 8 waves per SIMD */
    const u32 per_lane = 256;
    float best = 1e30f;
    for (int r = 0; r <= reps; r++) { /* launch 0 warms up */
        HIPCHK(c, hipEventRecord(e0, c->stream));
        hipLaunchKernelGGL(gather_rows_kernel, dim3(grid), dim3(256), 0, c->stream, tab, nrows, per_lane, sink);
        HIPCHK(c, hipEventRecord(e1, c->stream));
        HIPCHK(c, hipEventSynchronize(e1));
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, e0, e1));
        if (r > 0 && ms < best) best = ms;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipFree(tab);
    (void)hipFree(sink);
    *gb_per_s = (double)grid * 256.0 * per_lane * 64.0 / ((double)best * 1e-3) / 1e9;
    return DISCO_OK;
}

int disco_get_counters(disco_ctx *c, disco_counters *o)
{
    if (!c || !o) return DISCO_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    memset(o, 0, sizeof *o);
    o->n_reads = c->n;
    if (c->phase >= 1) {
        CHK(ensure_host_len(c));
        u64 q = 0;
        for (u64 i = c->q_lo; i < c->q_hi; i++) q += c->h_len[i] - c->k;
        o->probes = q;
    }
    o->kmer_hits = c->h_ctr[CTR_KMER_HITS];
    o->raw_hits = c->h_ctr[CTR_RAW_HITS];
    o->n_contained = c->n_contained;
    o->e_pre = c->phase >= 6 ? c->adj_total / 2 : 0;
    o->e_out = c->n_out;
    o->cap_bind_sites = c->h_ctr[CTR_CAP_SITES];
    o->asymmetric_pairs = c->asym_local;
    o->big_rows = c->big_rows;
    o->index_buckets = c->T;
    o->hbm_bytes = c->hbm_bytes;
    return DISCO_OK;
}

} /* extern "C" */

/* ================================================================================================================
 * multi-GPU flow (include/disco_hip.h "multi-GPU flow"; kernels: disco_dist.h; transport: disco_comm.h)
 *
 * One pass on rank r of G (own = [r*per, (r+1)*per) ∩ [0, n)):
 *   0. [flag] all-gather of the packed reads               every rank verifies candidates against any read
 *   1. index records of the OWN reads (no atomics)  →  all-to-all to the owner of their bucket range  →  the owner counts,
 *      scans and fills its shard straight into its slice of the global table  →  all-gather-v of the bkt / ent slices
 *   2. grouping + probe + verify of the own reads (unchanged kernels)
 *   3. reduce-scatter(MIN) of the containment keys, flags of the own range, all-gather of the bitmap
 *   4. edge selection of the own reads
 *   5. regular regime (no rank dropped a verified hit): rows of the neighbours a node's marking sweeps are requested from
 *      their owners, class-filtered 4-byte entries come back; marking; nodes that needed a row nobody had asked for are redone
 *      after a second, request-everything round
 *   6. surviving half-edges pushed to the owner of the smaller endpoint; emission
 *   order-dependent regime (some rank dropped a hit: per-k-mer cap, second hit to a destination): the whole adjacency is
 *   gathered and every rank completes, marks and judges all lists itself (exact, not scalable; never on BASELINE data)
 * ============================================================================================================== */

#define COMM_CHK(c, expr)                                                                        \
    do {                                                                                         \
        int rc_ = (expr);                                                                        \
        if (rc_ != DISCO_OK) return fail((c), rc_, "%s: %s", #expr, (c)->comm->err.c_str());    \
    } while (0)

static void dist_range(const disco_ctx *c, u64 n, u64 *per, u64 *lo, u64 *hi)
{
    const u64 G = c->comm ? (u64)c->comm->world : 1, r = c->comm ? (u64)c->comm->rank : 0;
    u64 p = (n + G - 1) / G;
    p = (p + 63) & ~63ull;
    if (p == 0) p = 64;
    *per = p;
    *lo = std::min(r * p, n);
    *hi = std::min(*lo + p, n);
}

/* partition items[0..n) into one segment per destination rank: out = segments in rank order, cnt[g] = items for rank g */
template <typename T, typename F>
static int route_items(disco_ctx *c, const T *items, u64 n, F owner, T *out, std::vector<u64> &cnt)
{
    const u32 G = (u32)c->comm->world;
    cnt.assign(G, 0);
    CHK(ensure(c, c->d_route, 2 * DIST_MAX_WORLD));
    HIPCHK(c, hipMemsetAsync(c->d_route, 0, 2 * DIST_MAX_WORLD * sizeof(u64), c->stream));
    if (n) hipLaunchKernelGGL((route_count_kernel<T, F>), dim3(flat_grid(c, n)), dim3(256), 0, c->stream, items, n, owner, G, c->d_route);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(cnt.data(), c->d_route, G * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    /* (the cursors are made on the device: the scattered segments are consumed by operations on this stream, nothing here waits for them) */
    hipLaunchKernelGGL(route_cursor_kernel, dim3(1), dim3(64), 0, c->stream, (const u64 *)c->d_route, G, c->d_route + DIST_MAX_WORLD);
    if (n) hipLaunchKernelGGL((route_scatter_kernel<T, F>), dim3(flat_grid(c, (n + ROUTE_ITEMS - 1) / ROUTE_ITEMS)), dim3(256), 0, c->stream, items, n, owner, G,
                              c->d_route + DIST_MAX_WORLD, out);
    HIPCHK(c, hipGetLastError());
    return DISCO_OK;
}

/* rcnt[p] = what rank p sends to this rank, from everybody's send counts */
static int exchange_counts(disco_ctx *c, const std::vector<u64> &scnt, std::vector<u64> &rcnt, std::vector<u64> *matrix = nullptr)
{
    const int G = c->comm->world;
    std::vector<u64> all((size_t)G * G);
    COMM_CHK(c, c->comm->host_all_gather((const unsigned long long *)scnt.data(), G, (unsigned long long *)all.data(), c->stream));
    rcnt.resize((size_t)G);
    for (int p = 0; p < G; p++) rcnt[(size_t)p] = all[(size_t)p * G + c->comm->rank];
    if (matrix) *matrix = std::move(all);
    return DISCO_OK;
}

/* all-to-all of item segments (elem bytes per item), both sides compact in rank order */
static int a2a_items(disco_ctx *c, int xid, const void *send, const std::vector<u64> &scnt, void *recv, const std::vector<u64> &rcnt, size_t elem)
{
    const int G = c->comm->world;
    std::vector<size_t> so((size_t)G), sc((size_t)G), ro((size_t)G), rc((size_t)G);
    size_t a = 0, b = 0;
    for (int p = 0; p < G; p++) {
        so[(size_t)p] = a;
        sc[(size_t)p] = scnt[(size_t)p] * elem;
        a += sc[(size_t)p];
        ro[(size_t)p] = b;
        rc[(size_t)p] = rcnt[(size_t)p] * elem;
        b += rc[(size_t)p];
        if (p != c->comm->rank) c->dinfo.bytes_sent[xid] += sc[(size_t)p];
    }
    const auto t0 = HClock::now();
    COMM_CHK(c, c->comm->all_to_all_v(send, so.data(), sc.data(), recv, ro.data(), rc.data(), c->stream));
    /* (stream ordered: whoever consumes the received blocks runs behind them on this stream. DISCO_DIST_TIME_EXCHANGES=1 waits here, so that
     * dinfo.ms shows the exchange itself and not the time to issue it) */
    if (c->time_exchanges) HIPCHK(c, hipStreamSynchronize(c->stream));
    c->dinfo.ms[xid] += ms_since(t0);
    return DISCO_OK;
}

static u64 vsum(const std::vector<u64> &v)
{
    u64 s = 0;
    for (u64 x : v) s += x;
    return s;
}

/* sum / max of a few host values over all ranks */
static int host_reduce(disco_ctx *c, u64 *vals, int n, bool take_max = false)
{
    const int G = c->comm->world;
    std::vector<u64> all((size_t)G * n);
    COMM_CHK(c, c->comm->host_all_gather((const unsigned long long *)vals, n, (unsigned long long *)all.data(), c->stream));
    for (int i = 0; i < n; i++) {
        u64 a = 0;
        for (int p = 0; p < G; p++) a = take_max ? std::max(a, all[(size_t)p * n + i]) : a + all[(size_t)p * n + i];
        vals[i] = a;
    }
    return DISCO_OK;
}

/* the rows and lengths of the own reads, from the ranks in whose home ranges they arrived (dist_deal_reads) */
template <int W>
static int dist_deal_rows(disco_ctx *c)
{
    typedef ReadItem<W> Item;
    const u64 nhome = c->home_hi - c->home_lo;
    const u64 per16 = (sizeof(Item) + 15) / 16; /* (d_x16a / d_x16b are arrays of 16-byte items) */
    CHK(ensure(c, c->d_x16a, std::max<u64>(2 * nhome * per16, 1)));
    Item *items = (Item *)c->d_x16a.p, *sorted = (Item *)(c->d_x16a + nhome * per16);
    if (nhome) hipLaunchKernelGGL(read_items_kernel<W>, dim3(flat_grid(c, nhome * (W + 1))), dim3(256), 0, c->stream, (const u64 *)c->d_reads, (const u16 *)c->d_len, c->S, c->home_lo, c->home_hi, items);
    HIPCHK(c, hipGetLastError());
    std::vector<u64> scnt, rcnt;
    RouteByReadItem<W> f{c->d_otab};
    CHK(route_items(c, items, nhome, f, sorted, scnt));
    CHK(exchange_counts(c, scnt, rcnt));
    const u64 nr = vsum(rcnt);
    if (nr != c->n_own) return fail(c, DISCO_E_STATE, "dealt reads: %llu rows arrive for %llu own reads", (unsigned long long)nr, (unsigned long long)c->n_own);
    CHK(ensure(c, c->d_x16b, std::max<u64>(nr * per16, 1)));
    CHK(a2a_items(c, DISCO_X_READS_DEALT, sorted, scnt, c->d_x16b, rcnt, sizeof(Item)));
    if (nr) hipLaunchKernelGGL(read_items_place_kernel<W>, dim3(flat_grid(c, nr * (W + 1))), dim3(256), 0, c->stream, (const Item *)c->d_x16b.p, nr, c->S, c->d_reads, c->d_len);
    HIPCHK(c, hipGetLastError());
    return DISCO_OK;
}

/* ---- 0'. ranks own loci: the reads of the pass are dealt to the ranks by their read-level minimizer -------------------------- */
/* Replaces needsProcessing (RMA/HashTable.cpp:1066-1087: a read is the business of the rank that owns its bucket) and the id
 * ranges of rounds 1-4. A rank's reads used to be a random G-th of every locus: nobody's neighbours in the processing order shared
 * candidates, rows or buckets any more (verify, probe and marking ran 1.5 x the time per read: profiles/r04_dist8_kernels.json) and
 * nearly every neighbour row was another rank's. Now: keys of the home range (read_keys_kernel) -> all-gather of the 4-byte keys ->
 * owner of every read = its key's share of the hash range (disco_key_owner: whole groups, no exchange of boundaries needed — the
 * grouping hash spreads the groups evenly) -> the own reads, grouped (the rank's processing order, d_order_own). From here on q_lo /
 * q_hi are POSITIONS of that list. Collective. */
static int dist_deal_reads(disco_ctx *c)
{
    DISCO_TRACE("dist_deal_reads");
    const u32 G = (u32)c->comm->world, r = (u32)c->comm->rank;
    const u64 hlo = c->home_lo, hhi = c->home_hi;
    CHK(ensure(c, c->d_okey, c->n_alloc));
    CHK(ensure(c, c->d_otab, c->n_alloc));
    DiscoView v = view(c);
    if (hhi > hlo) {
        if (v.m == RUNS_M) hipLaunchKernelGGL(read_keys_kernel<true>, dim3((unsigned)((hhi - hlo + 255) / 256)), dim3(256), 0, c->stream, v, hlo, hhi, c->d_okey);
        else hipLaunchKernelGGL(read_keys_kernel<false>, dim3((unsigned)((hhi - hlo + 255) / 256)), dim3(256), 0, c->stream, v, hlo, hhi, c->d_okey);
    }
    HIPCHK(c, hipGetLastError());
    {
        const auto t0 = HClock::now();
        COMM_CHK(c, c->comm->all_gather(c->d_okey + (u64)r * c->per, c->d_okey, c->per * sizeof(u32), c->stream));
        c->dinfo.bytes_sent[DISCO_X_KEYS] += (u64)(G - 1) * c->per * sizeof(u32);
        c->dinfo.ms[DISCO_X_KEYS] += ms_since(t0);
    }
    /* owners and the own reads (about n / G of them: sized for the whole job once — 4 bytes per read) */
    CHK(ensure(c, c->d_own_ids, std::max<u64>(c->n, 1)));
    CHK(ensure(c, c->d_list_n, 1));
    HIPCHK(c, hipMemsetAsync(c->d_list_n, 0, sizeof(u64), c->stream));
    /* the grouping of the own reads (the rank's processing order) counts its buckets in the same pass: how many buckets follows from
     * the number of own reads, which this pass produces — it is taken from the job's share n / G instead (the keys spread the reads to
     * 0.3 %); the number of buckets shapes the order, never a result */
    int obits = 16;
    const bool order_own = own_order_wanted(c, std::max<u64>(c->n / G, 1), &obits) && !getenv("DISCO_DIST_ORDER_TWO_PASSES");
    const u32 oshift = 32u - (u32)obits;
    if (order_own) {
        CHK(ensure(c, c->d_ocnt, (1ull << obits) + 1));
        CHK(ensure(c, c->d_oslot, std::max<u64>(c->n, 1))); /* (about n / G are used: sized like the list of own ids) */
        HIPCHK(c, hipMemsetAsync(c->d_ocnt, 0, ((1ull << obits) + 1) * sizeof(u32), c->stream));
    }
    if (c->n) hipLaunchKernelGGL(own_select_kernel, dim3((unsigned)std::min<u64>((c->n + OWN_TILE - 1) / OWN_TILE, (u64)c->n_cu * 16)), dim3(256), 0, c->stream, (const u32 *)c->d_okey, c->n, G, r,
                                 c->d_otab, c->d_own_ids, c->d_list_n, order_own ? c->d_ocnt : (u32 *)nullptr, order_own ? c->d_oslot : (u32 *)nullptr, oshift);
    HIPCHK(c, hipGetLastError());
    u64 n_own = 0;
    HIPCHK(c, hipMemcpyAsync(&n_own, c->d_list_n, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, counted_stream_sync(c->stream));
    c->n_own = n_own;
    c->loci = true;
    c->q_lo = 0;
    c->q_hi = n_own;
    /* the lengths and — for the index pass — the rows of the own reads: most of them arrived in other ranks' ranges. They come by an
     * all-to-all of their own, a seventh of what the all-gather of ALL reads moves (that one stays behind index build and probe: only
     * verify waits for it; it writes the same rows once more); shapes without a built variant wait for the all-gather here */
    if (c->wait_bulk_before_verify) {
        const int W = (int)((c->max_len + 31) / 32);
        if (W <= 5 && c->S >= 5 && !getenv("DISCO_DIST_NO_DEAL_ROWS")) CHK(dist_deal_rows<5>(c));
        else if (W <= 8 && c->S >= 8 && !getenv("DISCO_DIST_NO_DEAL_ROWS")) CHK(dist_deal_rows<8>(c));
        else {
            HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_bulk, 0));
            c->wait_bulk_before_verify = false;
        }
    }
    /* the processing order: the own reads grouped by key (disco_probe's grouping, over the list) */
    CHK(ensure(c, c->d_order_own, std::max<u64>(n_own, 1)));
    ph_begin(c, DISCO_PH_ORDER);
    int obits2 = 16;
    const bool order_two = !order_own && own_order_wanted(c, n_own, &obits2); /* (DISCO_DIST_ORDER_TWO_PASSES: the counting pass of rounds 5 as a pass of its own) */
    if ((order_own && n_own) || order_two) {
        const int ob = order_own ? obits : obits2;
        const u64 order_buckets = 1ull << ob;
        const u32 oshift = 32u - (u32)ob;
        if (order_two) {
            CHK(ensure(c, c->d_ocnt, order_buckets + 1));
            CHK(ensure(c, c->d_oslot, n_own));
            HIPCHK(c, hipMemsetAsync(c->d_ocnt, 0, (order_buckets + 1) * sizeof(u32), c->stream));
            hipLaunchKernelGGL(order_count_list_kernel, dim3(flat_grid(c, n_own)), dim3(256), 0, c->stream, (const u32 *)c->d_okey, (const u32 *)c->d_own_ids, n_own, G, r, oshift, c->d_ocnt, c->d_oslot);
        }
        CHK((scan_exclusive<u32, u32>(c, c->d_ocnt, order_buckets + 1, c->d_ocnt, false, nullptr)));
        hipLaunchKernelGGL(order_scatter_list_kernel, dim3(flat_grid(c, n_own)), dim3(256), 0, c->stream, (const u32 *)c->d_okey, (const u32 *)c->d_own_ids, (const u32 *)c->d_oslot,
                           (const u32 *)c->d_ocnt, n_own, G, r, oshift, (const u16 *)c->d_len, c->d_order_own);
    } else if (n_own)
        hipLaunchKernelGGL(order_pack_list_kernel, dim3(flat_grid(c, n_own)), dim3(256), 0, c->stream, (const u32 *)c->d_own_ids, n_own, (const u16 *)c->d_len, c->d_order_own);
    ph_end(c, DISCO_PH_ORDER);
    HIPCHK(c, hipGetLastError());
    c->d_order_used = c->d_order_own;
    c->order_counted = false;
    c->dinfo.own_reads = n_own;
    return DISCO_OK;
}

/* ---- 1. hash-partitioned index build ------------------------------------------------------------------------------- */
static int dist_build_index(disco_ctx *c)
{
    DISCO_TRACE("dist_build_index");
    const u32 G = (u32)c->comm->world, r = (u32)c->comm->rank;
    const u64 nloc = c->q_hi - c->q_lo;
    const int logT = size_bucket_table(c);
    const u64 T = c->T;
    auto blo_of = [&](u64 g) { return (g * T + G - 1) / G; };
    const u64 blo = blo_of(r), bhi = blo_of(r + 1);
    const bool part = c->part_index;
    if (!part) { /* (partitioned: the slices are sized below, once the records have arrived) */
        CHK(ensure(c, c->d_bkt, T + 1));
        CHK(ensure(c, c->d_ent, 2 * c->n));
    }
    CHK(ensure(c, c->d_okey, c->loci ? c->n_alloc : c->n));
    CHK(ensure(c, c->d_rec, std::max<u64>(2 * nloc, 1)));
    c->adj_imported = false;
    ph_begin(c, DISCO_PH_INDEX);
    DiscoView v = view(c);
    IndexCountPlan pl;
    IndexRecOut rec_out; /* 16-byte records without a slot: they travel to the rank that owns their bucket and are counted there */
    rec_out.form = INDEX_RECORDS;
    rec_out.rec = c->d_rec.p;
    if (c->loci) { /* the own list: records and minimizer runs by POSITION in the processing order */
        CHK(index_count_plan(c, v, 0, c->n_own, &pl, c->d_order_own));
        CHK(index_count_chunk(c, v, pl, rec_out, 0, c->n_own));
    } else {
        CHK(index_count_plan(c, v, c->q_lo, c->q_hi, &pl));
        CHK(index_count_chunk(c, v, pl, rec_out, c->q_lo, c->q_hi));
        if (c->two_class && nloc) {
            /* the long reads of the rank's range — long_ids is ascending, ovf[i] counts the long reads in front of read i: they are the
             * x in [ovf[q_lo], ovf[q_hi]) — from their full rows; records by read id from q_lo (the kernel indexes rec by read id) */
            u32 xb[2] = {0, (u32)c->n_long};
            HIPCHK(c, hipMemcpyAsync(&xb[0], c->d_ovf + c->q_lo, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
            if (c->q_hi < c->n) HIPCHK(c, hipMemcpyAsync(&xb[1], c->d_ovf + c->q_hi, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (xb[1] > xb[0]) {
                const IndexRecOut rec_by_id = rec_out.from_read(-(ptrdiff_t)c->q_lo); /* rec_by_id.rec[2 i] = the record of read i (never touched outside [q_lo, q_hi)) */
                u32 *oslot_by_id = pl.oslot ? pl.oslot - (ptrdiff_t)c->q_lo : nullptr; /* (the grouping's slots: by read id too) */
                CHK(index_count_long(c, v, pl, rec_by_id, oslot_by_id, xb[0], xb[1]));
            }
        }
    }
    /* records -> owner of their bucket range */
    CHK(ensure(c, c->d_x16a, std::max<u64>(2 * nloc, 1)));
    std::vector<u64> scnt, rcnt, matrix;
    RouteByBucket f{logT, G};
    CHK(route_items(c, c->d_rec.p, 2 * nloc, f, c->d_x16a.p, scnt));
    CHK(exchange_counts(c, scnt, rcnt, &matrix));
    const u64 nrec = vsum(rcnt);
    CHK(ensure(c, c->d_x16b, std::max<u64>(nrec, 1)));
    CHK(a2a_items(c, DISCO_X_INDEX_RECORDS, c->d_x16a, scnt, c->d_x16b, rcnt, sizeof(ulonglong2)));
    /* my bucket range and the position of my records in the global record array (shards in rank order) */
    std::vector<u64> shard((size_t)G, 0);
    for (u32 p = 0; p < G; p++)
        for (u32 q = 0; q < G; q++) shard[q] += matrix[(size_t)p * G + q];
    u64 base = 0;
    for (u32 q = 0; q < r; q++) base += shard[q];
    if (shard[r] != nrec) return fail(c, DISCO_E_STATE, "index shard: %llu records received, %llu announced", (unsigned long long)nrec, (unsigned long long)shard[r]);
    if (vsum(shard) != 2 * c->n) return fail(c, DISCO_E_STATE, "index: %llu records over all ranks, expected %llu", (unsigned long long)vsum(shard), (unsigned long long)(2 * c->n));
    if (part) {
        /* the index STAYS partitioned: this rank's slice of the bucket table (bhi - blo + 1 entries, bucket b at [b - blo]) and its
         * records (positions inside the slice) are all it ever holds; the lookups come to it (dist_partitioned_probe) */
        CHK(ensure(c, c->d_bkt, bhi - blo + 1));
        CHK(ensure(c, c->d_ent, std::max<u64>(nrec, 1)));
        u32 *bkt0 = c->d_bkt - blo; /* indexed by global bucket number */
        HIPCHK(c, hipMemsetAsync(c->d_bkt, 0, (bhi - blo + 1) * sizeof(u32), c->stream));
        if (nrec) hipLaunchKernelGGL(shard_count_kernel, dim3(flat_grid(c, nrec)), dim3(256), 0, c->stream, c->d_x16b, nrec, bkt0);
        CHK((scan_exclusive<u32, u32>(c, c->d_bkt, bhi - blo + 1, c->d_bkt, false, nullptr)));
        if (nrec) hipLaunchKernelGGL(index_fill_kernel, dim3(flat_grid(c, nrec)), dim3(256), 0, c->stream, nrec, c->d_x16b, bkt0, c->d_ent);
        HIPCHK(c, hipGetLastError());
        c->part_blo = blo;
        c->part_bhi = bhi;
        c->part_nrec = nrec;
        ph_end(c, DISCO_PH_INDEX);
        c->phase = 2;
        return DISCO_OK;
    }
    if (bhi > blo) HIPCHK(c, hipMemsetAsync(c->d_bkt + blo, 0, (bhi - blo) * sizeof(u32), c->stream));
    if (nrec) hipLaunchKernelGGL(shard_count_kernel, dim3(flat_grid(c, nrec)), dim3(256), 0, c->stream, c->d_x16b, nrec, c->d_bkt);
    if (bhi > blo) {
        CHK((scan_exclusive<u32, u32>(c, c->d_bkt + blo, bhi - blo, c->d_bkt + blo, false, nullptr)));
        if (base) hipLaunchKernelGGL(add_u32_kernel, dim3(flat_grid(c, bhi - blo)), dim3(256), 0, c->stream, c->d_bkt + blo, bhi - blo, (u32)base);
    }
    if (nrec) hipLaunchKernelGGL(index_fill_kernel, dim3(flat_grid(c, nrec)), dim3(256), 0, c->stream, nrec, c->d_x16b, c->d_bkt, c->d_ent);
    const u32 total = (u32)(2 * c->n);
    HIPCHK(c, hipMemcpyAsync(c->d_bkt + T, &total, sizeof(u32), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    /* shards -> everybody (in place: every rank wrote its slices where they belong) */
    {
        std::vector<size_t> off((size_t)G), cnt((size_t)G);
        const auto t0 = HClock::now();
        for (u32 p = 0; p < G; p++) {
            off[p] = blo_of(p) * sizeof(u32);
            cnt[p] = (blo_of(p + 1) - blo_of(p)) * sizeof(u32);
        }
        c->dinfo.bytes_sent[DISCO_X_INDEX_SHARDS] += (u64)(G - 1) * cnt[r]; /* (rounds 1-4 added cnt[r] inside the loop, before it was set for p < r: ranks above 0 under-reported) */
        COMM_CHK(c, c->comm->all_gather_v(c->d_bkt + blo, c->d_bkt, off.data(), cnt.data(), c->stream));
        size_t a = 0;
        for (u32 p = 0; p < G; p++) {
            off[p] = a;
            cnt[p] = shard[p] * sizeof(u64);
            a += cnt[p];
        }
        c->dinfo.bytes_sent[DISCO_X_INDEX_SHARDS] += (u64)(G - 1) * cnt[r];
        COMM_CHK(c, c->comm->all_gather_v(c->d_ent + base, c->d_ent, off.data(), cnt.data(), c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->dinfo.ms[DISCO_X_INDEX_SHARDS] += ms_since(t0);
    }
    ph_end(c, DISCO_PH_INDEX);
    c->phase = 2;
    return DISCO_OK;
}

/* ---- 2'. the probe against an index that stays partitioned: lookups to the owners, matching records back --------------------- */
/* (kernels and formats: disco_dist.h "the index that STAYS partitioned"). Fills the hit buffer and the per-read headers exactly as
 * probe_runs_kernel does for the replicated index: rows by read, headers by position in the processing order. Collective. */
static int dist_partitioned_probe(disco_ctx *c)
{
    DISCO_TRACE("dist_partitioned_probe");
    const u32 G = (u32)c->comm->world, r = (u32)c->comm->rank;
    const u64 lo = c->q_lo, nloc = c->q_hi - c->q_lo;
    DiscoView v = view(c);
    const int nf = v.ks - v.m + 1;
    const bool seeded = c->k != c->ks; /* (instantiations of their own: without a seed the kernels are what they were) */
    const bool have_runs = c->runs_lpr != 0 && c->runs_lo == lo && c->runs_n == nloc; /* (every rank decides alike: the shape of the JOB) */
    int logT = 0;
    while ((1ull << logT) < c->T) ++logT;
    /* 1. queries. With the minimizer runs of the index pass: one per run (count, then fill), reads with an unusable run list the long
     *    way; without them (windows other than 17 m-mers, reads beyond 256 bases) every read the long way */
    CHK(ensure(c, c->d_list_n, 1));
    u32 *d_nslow = c->d_n_slow;
    auto make = [&](ulonglong2 *out, bool collect_slow) {
        const int grid = flat_grid(c, nloc * (u64)c->runs_lpr);
        u32 *slow = collect_slow ? (u32 *)c->d_slow_list.p : nullptr;
        const u32 cap = c->d_slow_list.cap * 2; /* (the list's u64 slots hold two read indices each) */
        auto fn = seeded ? (c->runs_lpr == 16 ? pq_make_kernel<16, true> : pq_make_kernel<32, true>) : (c->runs_lpr == 16 ? pq_make_kernel<16> : pq_make_kernel<32>);
        hipLaunchKernelGGL(fn, dim3(grid), dim3(256), 0, c->stream, v, (const u32 *)c->d_runs, lo, c->q_hi, r, out, c->d_list_n, slow, cap, d_nslow);
    };
    u64 nq_fast = 0, n_slow = 0;
    const u32 *slow = nullptr; /* null: every read of the range */
    if (have_runs) {
        u32 ns = 0;
        for (int attempt = 0;; attempt++) { /* the list of reads without a usable run list: sized by a first try */
            const u32 want = attempt ? ns / 2 + 1024 : (u32)std::min<u64>(nloc, nloc / 128 + 1024);
            if (want > c->d_slow_list.cap) CHK(ensure(c, c->d_slow_list, want));
            HIPCHK(c, hipMemsetAsync(c->d_list_n, 0, sizeof(u64), c->stream));
            HIPCHK(c, hipMemsetAsync(d_nslow, 0, sizeof(u32), c->stream));
            if (nloc) make(nullptr, true);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(&nq_fast, c->d_list_n, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(&ns, d_nslow, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (ns <= c->d_slow_list.cap * 2 || attempt) break;
        }
        if (ns > c->d_slow_list.cap * 2) return fail(c, DISCO_E_CAPACITY, "dist_partitioned_probe: slow list could not be sized");
        n_slow = ns;
        slow = (const u32 *)c->d_slow_list.p;
    } else
        n_slow = nloc;
    /* the long way: queries per read, scan, fill behind the fast ones */
    u64 nq_slow = 0, nqs = 0;
    { /* (the two buffers of the long way are gone before the exchange below) */
    LocalBuf<u32> slow_cnt(c);
    LocalBuf<u64> slow_start(c);
    if (n_slow) {
        CHK(ensure(c, slow_cnt, n_slow));
        CHK(ensure(c, slow_start, n_slow + 1));
        if (seeded) hipLaunchKernelGGL((pq_slow_kernel<true, true>), dim3(flat_grid(c, n_slow, 64)), dim3(64), 0, c->stream, v, slow, n_slow, lo, r, slow_cnt, (const u64 *)nullptr, (ulonglong2 *)nullptr);
        else if (c->ks > 64) hipLaunchKernelGGL(pq_slow_kernel<true>, dim3(flat_grid(c, n_slow, 64)), dim3(64), 0, c->stream, v, slow, n_slow, lo, r, slow_cnt, (const u64 *)nullptr, (ulonglong2 *)nullptr);
        else hipLaunchKernelGGL(pq_slow_kernel<false>, dim3(flat_grid(c, n_slow, 64)), dim3(64), 0, c->stream, v, slow, n_slow, lo, r, slow_cnt, (const u64 *)nullptr, (ulonglong2 *)nullptr);
        CHK((scan_exclusive<u32, u64>(c, slow_cnt, n_slow, slow_start, false, &nq_slow)));
    }
    nqs = nq_fast + nq_slow;
    CHK(ensure(c, c->d_x16a, std::max<u64>(2 * nqs, 1))); /* flat list | partitioned by owner */
    HIPCHK(c, hipMemsetAsync(c->d_list_n, 0, sizeof(u64), c->stream));
    if (have_runs && nloc) make(c->d_x16a, false);
    if (n_slow) {
        if (seeded) hipLaunchKernelGGL((pq_slow_kernel<true, true>), dim3(flat_grid(c, n_slow, 64)), dim3(64), 0, c->stream, v, slow, n_slow, lo, r, slow_cnt, (const u64 *)slow_start, c->d_x16a + nq_fast);
        else if (c->ks > 64) hipLaunchKernelGGL(pq_slow_kernel<true>, dim3(flat_grid(c, n_slow, 64)), dim3(64), 0, c->stream, v, slow, n_slow, lo, r, slow_cnt, (const u64 *)slow_start, c->d_x16a + nq_fast);
        else hipLaunchKernelGGL(pq_slow_kernel<false>, dim3(flat_grid(c, n_slow, 64)), dim3(64), 0, c->stream, v, slow, n_slow, lo, r, slow_cnt, (const u64 *)slow_start, c->d_x16a + nq_fast);
    }
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return fail(c, DISCO_E_HIP, "dist_partitioned_probe: query kernels failed");
    }
    c->slow_rows = have_runs ? n_slow : 0;
    /* 2. queries -> owners of their buckets */
    std::vector<u64> scnt, rcnt;
    RouteByBucket fb{logT, G};
    ulonglong2 *q_sorted = c->d_x16a + nqs;
    CHK(route_items(c, c->d_x16a.p, nqs, fb, q_sorted, scnt));
    CHK(exchange_counts(c, scnt, rcnt));
    const u64 nq_in = vsum(rcnt);
    CHK(ensure(c, c->d_x16b, std::max<u64>(nq_in, 1)));
    CHK(a2a_items(c, DISCO_X_QUERIES, q_sorted, scnt, c->d_x16b, rcnt, sizeof(ulonglong2)));
    /* 3. the owner answers: hits per query, scan, fill */
    CHK(ensure(c, c->d_deg_tmp, std::max<u64>(nq_in, 1)));
    CHK(ensure(c, c->d_pq_start, nq_in + 1));
    const u32 *bkt = c->d_bkt;
    u64 n_hits_out = 0;
    auto answer_count = seeded ? pq_answer_kernel<false, true> : pq_answer_kernel<false, false>;
    auto answer_fill = seeded ? pq_answer_kernel<true, true> : pq_answer_kernel<true, false>;
    if (nq_in) hipLaunchKernelGGL(answer_count, dim3(flat_grid(c, nq_in)), dim3(256), 0, c->stream, (const ulonglong2 *)c->d_x16b, nq_in, bkt, (const u64 *)c->d_ent, c->part_blo, c->per,
                                  nf, c->k - c->ks, c->d_deg_tmp, (const u64 *)nullptr, (ulonglong2 *)nullptr);
    CHK((scan_exclusive<u32, u64>(c, c->d_deg_tmp, nq_in, c->d_pq_start, false, &n_hits_out)));
    /* hits: flat list | partitioned by requester — in the send buffer (the queries it held have been answered into counts) */
    CHK(ensure_keep(c, c->d_x16a, std::max<u64>(2 * n_hits_out, 1), 0));
    if (nq_in) hipLaunchKernelGGL(answer_fill, dim3(flat_grid(c, nq_in)), dim3(256), 0, c->stream, (const ulonglong2 *)c->d_x16b, nq_in, bkt, (const u64 *)c->d_ent, c->part_blo, c->per,
                                  nf, c->k - c->ks, c->d_deg_tmp, (const u64 *)c->d_pq_start, c->d_x16a);
    HIPCHK(c, hipGetLastError());
    /* 4. hits -> the reads' owners */
    ulonglong2 *h_sorted = c->d_x16a + n_hits_out;
    RouteByHitRank fh;
    CHK(route_items(c, c->d_x16a.p, n_hits_out, fh, h_sorted, scnt));
    CHK(exchange_counts(c, scnt, rcnt));
    const u64 n_hits = vsum(rcnt);
    CHK(ensure(c, c->d_x16b, std::max<u64>(n_hits, 1)));
    CHK(a2a_items(c, DISCO_X_HITS, h_sorted, scnt, c->d_x16b, rcnt, sizeof(ulonglong2)));
    /* 5. rows of the hit buffer (exactly sized), headers by read and by position in the processing order */
    if (n_hits + 65536 > c->d_hits.cap) CHK(ensure(c, c->d_hits, n_hits + n_hits / 8 + 65536));
    CHK(ensure(c, c->d_deg_tmp, std::max<u64>(2 * nloc, 1))); /* counts | cursors of the own reads */
    CHK(ensure(c, c->d_pq_start, nloc + 1));
    HIPCHK(c, hipMemsetAsync(c->d_deg_tmp, 0, std::max<u64>(2 * nloc, 1) * sizeof(u32), c->stream));
    if (n_hits) hipLaunchKernelGGL(pq_rows_count_kernel, dim3(flat_grid(c, n_hits)), dim3(256), 0, c->stream, (const ulonglong2 *)c->d_x16b, n_hits, c->d_deg_tmp);
    u64 placed = 0;
    CHK((scan_exclusive<u32, u64>(c, c->d_deg_tmp, nloc, c->d_pq_start, false, &placed)));
    if (placed != n_hits) return fail(c, DISCO_E_STATE, "dist_partitioned_probe: %llu hits received, %llu placed", (unsigned long long)n_hits, (unsigned long long)placed);
    if (n_hits) hipLaunchKernelGGL(pq_rows_place_kernel, dim3(flat_grid(c, n_hits)), dim3(256), 0, c->stream, (const ulonglong2 *)c->d_x16b, n_hits, (const u64 *)c->d_pq_start, c->d_deg_tmp + nloc,
                                   c->d_hits);
    if (nloc) {
        hipLaunchKernelGGL(pq_rows_meta_kernel, dim3(flat_grid(c, nloc)), dim3(256), 0, c->stream, c->d_order_used, lo, nloc, (const u16 *)c->d_len, (const u64 *)c->d_pq_start,
                           (const u32 *)c->d_deg_tmp, c->d_row_start, c->d_row_cnt, c->d_meta_ord);
        CHK(zero_counter(c, CTR_MAX_ROW));
        hipLaunchKernelGGL(max_u32_kernel, dim3(flat_grid(c, nloc)), dim3(256), 0, c->stream, (const u32 *)c->d_deg_tmp, nloc, c->d_ctr + CTR_MAX_ROW);
    }
    HIPCHK(c, hipGetLastError());
    c->hits_used = n_hits;
    c->big_rows = 0;
    return DISCO_OK;
}

/* ---- 3. containment: smallest key wins across ranks, flags of the own range, bitmap to everybody -------------------- */
static int dist_mark_contained(disco_ctx *c)
{
    DISCO_TRACE("dist_mark_contained");
    const u32 G = (u32)c->comm->world;
    /* (the flags of an id range are fixed by the rank whose reads arrived in it, whoever processes them: best[] is a table by read id) */
    const u64 lo = c->home_lo, nloc = c->home_hi - c->home_lo, per = c->per;
    CHK(ensure(c, c->d_contained, c->n_alloc));
    CHK(ensure(c, c->d_cbits, c->n_alloc / 64 + 1));
    const auto t0 = HClock::now();
    const u64 r = (u64)c->comm->rank;
    /* Who is contained decides everything that follows in the pass (edge selection, the second verify pass); by WHOM — the smallest key
     * over the ranks — only the row that is written at the end. So the pass exchanges bitmaps (every rank's "has a key" bits: n / 8
     * bytes per rank instead of 8 n) and the keys' reduce-scatter runs behind it, on the second communicator and stream: 1.0 ms of
     * link time at G = 8 / 50 M reads that nothing used to hide. DISCO_DIST_KEYS_ON_PATH=1 (every rank alike), one communicator: as before */
    if (c->comm_bulk && !getenv("DISCO_DIST_ONE_COMM") && !getenv("DISCO_DIST_KEYS_ON_PATH")) {
        const u64 words = c->n_alloc / 64;
        CHK(ensure(c, c->d_cb_all, std::max<u64>(words * G, 1)));
        if (!c->ev_keys) {
            HIPCHK(c, hipEventCreateWithFlags(&c->ev_keys, hipEventDisableTiming));
            HIPCHK(c, hipEventCreateWithFlags(&c->ev_keys_go, hipEventDisableTiming));
        }
        CHK(zero_counter(c, CTR_N_CONTAINED));
        ph_begin(c, DISCO_PH_CONTAIN);
        u64 *mine = c->d_cb_all + r * words;
        if (c->n_alloc) hipLaunchKernelGGL(has_key_bits_kernel, dim3(flat_grid(c, c->n_alloc)), dim3(256), 0, c->stream, (const u64 *)c->d_best, c->n_alloc, mine);
        HIPCHK(c, hipGetLastError());
        COMM_CHK(c, c->comm->all_gather(mine, c->d_cb_all, words * 8, c->stream));
        c->dinfo.bytes_sent[DISCO_X_CONTAIN] += (u64)(G - 1) * words * 8;
        HIPCHK(c, hipMemsetAsync(c->d_contained, 0, std::max<u64>(c->n_alloc, 1), c->stream));
        if (words) hipLaunchKernelGGL(or_bits_kernel, dim3(flat_grid(c, words)), dim3(256), 0, c->stream, (const u64 *)c->d_cb_all, G, words, c->d_cbits, r * per / 64, (r + 1) * per / 64, c->d_contained, c->d_ctr); /* (r per, not home_lo: a rank behind the last read has home_lo = n, in the middle of another rank's word) */
        HIPCHK(c, hipGetLastError());
        ph_end(c, DISCO_PH_CONTAIN);
        /* the keys, behind everything the stream has done so far (verify wrote them) */
        HIPCHK(c, hipEventRecord(c->ev_keys_go, c->stream));
        HIPCHK(c, hipStreamWaitEvent(c->bulk_stream, c->ev_keys_go, 0));
        if (c->comm_bulk->reduce_scatter_min_i64(c->d_best, per, c->bulk_stream) != DISCO_OK) return fail(c, DISCO_E_HIP, "containment keys: %s", c->comm_bulk->err.c_str());
        HIPCHK(c, hipEventRecord(c->ev_keys, c->bulk_stream));
        c->keys_pending = true;
        c->dinfo.bytes_sent[DISCO_X_CONTAIN_KEYS] += (u64)(G - 1) * per * 8;
        CHK(read_counters(c));
        ph_collect(c);
        c->dinfo.ms[DISCO_X_CONTAIN] += ms_since(t0);
        c->n_contained = c->h_ctr[CTR_N_CONTAINED]; /* home range: what disco_fetch_contained returns */
        c->phase = 4;
        return DISCO_OK;
    }
    COMM_CHK(c, c->comm->reduce_scatter_min_i64(c->d_best, per, c->stream));
    c->dinfo.bytes_sent[DISCO_X_CONTAIN] += (u64)(G - 1) * per * 8;
    CHK(zero_counter(c, CTR_N_CONTAINED));
    ph_begin(c, DISCO_PH_CONTAIN);
    HIPCHK(c, hipMemsetAsync(c->d_contained, 0, std::max<u64>(c->n_alloc, 1), c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_cbits + r * per / 64, 0, per / 8, c->stream));
    if (nloc) hipLaunchKernelGGL(contain_flags_kernel, dim3(flat_grid(c, nloc)), dim3(256), 0, c->stream, c->d_best + lo, nloc, c->d_contained + lo, c->d_cbits + lo / 64, c->d_ctr);
    HIPCHK(c, hipGetLastError());
    COMM_CHK(c, c->comm->all_gather(c->d_cbits + r * per / 64, c->d_cbits, per / 8, c->stream));
    c->dinfo.bytes_sent[DISCO_X_CONTAIN] += (u64)(G - 1) * per / 8;
    ph_end(c, DISCO_PH_CONTAIN);
    CHK(read_counters(c));
    ph_collect(c);
    c->dinfo.ms[DISCO_X_CONTAIN] += ms_since(t0);
    c->n_contained = c->h_ctr[CTR_N_CONTAINED]; /* own range: what disco_fetch_contained returns */
    c->phase = 4;
    return DISCO_OK;
}

/* ---- 5. neighbour rows on request ------------------------------------------------------------------------------------ */
/* room for `need` more entries of fetched rows behind the rank's own rows (and behind the nadj_used entries fetched so far) in the array
 * that holds them — the hit buffer (64 slots per read allotted, 36 used at 30 x: the tail is there) or the merged rows; *base = where they go */
static int adj_tail_reserve(disco_ctx *c, u64 need, u64 *base)
{
    const bool in_hits = c->d_adj == c->d_hits;
    const u64 used = (in_hits ? c->hits_used : c->adj_total) + c->nadj_used;
    /* test hook: the array counts as full — every call with something to place moves it (the path a probe that sizes the buffer exactly takes) */
    const bool tight = getenv("DISCO_TEST_TIGHT_TAIL") != nullptr && need != 0;
    const u64 tight_cap = used + need + (used + need) / 8; /* (ensure_keep's size, for an array that is large enough on paper) */
    if (in_hits) {
        if (tight) CHK(move_keep(c, c->d_hits, tight_cap, used));
        else if (used + need > c->d_hits.cap) CHK(ensure_keep(c, c->d_hits, used + need, used));
        c->d_adj = c->d_hits;
    } else {
        if (c->d_adj != c->d_adj_own) return fail(c, DISCO_E_STATE, "neighbour rows: the adjacency is in neither of the buffers that can grow");
        if (tight) CHK(move_keep(c, c->d_adj_own, tight_cap, used));
        else if (used + need > c->d_adj_own.cap) CHK(ensure_keep(c, c->d_adj_own, used + need, used));
        c->d_adj = c->d_adj_own;
    }
    *base = used;
    return DISCO_OK;
}

/* ---- 5. neighbour rows on request (the exchange) ---------------------------------------------------------------------- */
/* one request round: the flat list of requested nodes in d_req_flat -> their rows behind the own rows (rows_place_kernel), their reference words set */
static int dist_fetch_rows(disco_ctx *c, u64 n_flat)
{
    DISCO_TRACE("dist_fetch_rows");
    const u32 G = (u32)c->comm->world;
    std::vector<u64> scnt, rcnt;
    CHK(ensure(c, c->d_req_s, std::max<u64>(n_flat, 1)));
    RouteByRowRequest f{c->per, c->loci ? c->d_otab : nullptr};
    CHK(route_items(c, c->d_req_flat.p, n_flat, f, c->d_req_s.p, scnt));
    CHK(exchange_counts(c, scnt, rcnt));
    const u64 nrq = vsum(rcnt);
    CHK(ensure(c, c->d_req_r, std::max<u64>(nrq, 1)));
    CHK(a2a_items(c, DISCO_X_ROW_REQUESTS, c->d_req_s, scnt, c->d_req_r, rcnt, sizeof(u32)));
    /* the owner's side: degree of every requested row, positions, entries */
    CHK(ensure(c, c->d_rdeg_s, std::max<u64>(nrq, 1)));
    CHK(ensure(c, c->d_rpos, std::max<u64>(std::max(nrq, n_flat), 1) + 1));
    const int rgrid = (int)std::max<u64>(std::min<u64>((nrq + 3) / 4, (u64)c->n_cu * 32), 1);
    if (nrq) hipLaunchKernelGGL(tr_respond_deg_kernel, dim3(flat_grid(c, nrq)), dim3(256), 0, c->stream, c->d_req_r, nrq, c->d_adj_ref, c->d_rdeg_s);
    HIPCHK(c, hipGetLastError());
    u64 total_s = 0;
    CHK((scan_exclusive<u32, u64>(c, c->d_rdeg_s, nrq, c->d_rpos, true, &total_s)));
    std::vector<u64> ecnt_s((size_t)G, 0), ecnt_r;
    {   /* entries per requester = differences of the positions at the segment boundaries */
        std::vector<u64> bpos((size_t)G + 1, 0);
        u64 a = 0;
        for (u32 p = 0; p < G; p++) {
            if (nrq) HIPCHK(c, hipMemcpyAsync(&bpos[p], c->d_rpos + a, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
            a += rcnt[p];
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));
        bpos[G] = total_s;
        for (u32 p = 0; p < G; p++) ecnt_s[p] = bpos[p + 1] - bpos[p];
    }
    CHK(ensure(c, c->d_rdata_s, std::max<u64>(total_s, 1)));
    if (nrq) hipLaunchKernelGGL(tr_respond_kernel, dim3(rgrid), dim3(64), 0, c->stream, c->d_req_r, nrq, c->d_adj_ref, c->d_adj, c->d_rpos, c->d_rdata_s);
    HIPCHK(c, hipGetLastError());
    /* degrees back (same segmentation as the requests, reversed), then the entries. How many entries every owner sends follows from
     * the degrees themselves: the requester sums them per segment (positions at the segment boundaries) — no exchange of counts */
    CHK(ensure(c, c->d_rdeg_r, std::max<u64>(n_flat, 1)));
    CHK(a2a_items(c, DISCO_X_ROW_REQUESTS, c->d_rdeg_s, rcnt, c->d_rdeg_r, scnt, sizeof(u32)));
    u64 total_r = 0;
    CHK((scan_exclusive<u32, u64>(c, c->d_rdeg_r, n_flat, c->d_rpos, true, &total_r))); /* (d_rpos: the owner's positions were consumed by tr_respond_kernel above) */
    ecnt_r.assign((size_t)G, 0);
    {
        std::vector<u64> bpos((size_t)G + 1, 0);
        u64 a = 0;
        for (u32 p = 0; p < G; p++) {
            if (n_flat) HIPCHK(c, hipMemcpyAsync(&bpos[p], c->d_rpos + a, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
            a += scnt[p];
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));
        bpos[G] = total_r;
        for (u32 p = 0; p < G; p++) ecnt_r[p] = bpos[p + 1] - bpos[p];
    }
    /* the rows that arrive (4-byte entries) ... */
    CHK(ensure(c, c->d_nadj32_own, std::max<u64>(total_r, 1)));
    CHK(a2a_items(c, DISCO_X_ROW_DATA, c->d_rdata_s, ecnt_s, c->d_nadj32_own, ecnt_r, sizeof(u32)));
    /* ... go behind the own rows, as 8-byte entries under the nodes' reference words */
    u64 base = 0;
    CHK(adj_tail_reserve(c, total_r, &base));
    if (n_flat) hipLaunchKernelGGL(rows_place_kernel, dim3((int)std::max<u64>(std::min<u64>((n_flat + 3) / 4, (u64)c->n_cu * 32), 1)), dim3(64), 0, c->stream, c->d_req_s, n_flat, c->d_rdeg_r, c->d_rpos,
                                   (const u32 *)c->d_nadj32_own, base, c->d_adj, c->d_adj_ref);
    HIPCHK(c, hipGetLastError());
    c->nadj_used += total_r;
    return DISCO_OK;
}

static int dist_transitive_mark(disco_ctx *c)
{
    DISCO_TRACE("dist_transitive_mark");
    const u64 nloc = c->q_hi - c->q_lo; /* own nodes (an id range, or the positions of the own list) */
    const OwnSet own = own_set(c);
    /* the reference words of other ranks' nodes are 0 = "not fetched" (edge selection cleared the table and wrote the own nodes' words; a
     * merge rebuilt it from degrees: 0 for every node of another rank); one bit per node: somebody on this rank has asked for its row */
    CHK(ensure(c, c->d_asked, c->n / 32 + 2));
    HIPCHK(c, hipMemsetAsync(c->d_asked, 0, (c->n / 32 + 2) * sizeof(u32), c->stream));
    c->nadj_used = 0; /* fetched rows: behind the own rows (adj_tail_reserve) */
    /* round 1: slot 0 and the first slot on the other side of every register-resident node */
    CHK(ensure(c, c->d_list_n, 1));
    CHK(ensure(c, c->d_req_flat, 2 * nloc + 64));
    HIPCHK(c, hipMemsetAsync(c->d_list_n, 0, sizeof(u64), c->stream));
    CHK(zero_counter(c, CTR_OVERFLOW));
    ph_begin(c, DISCO_PH_CSR);
    if (nloc) hipLaunchKernelGGL(tr_request_first_kernel, dim3((int)std::max<u64>(std::min<u64>((nloc + 63) / 64, (u64)c->n_cu * 32), 1)), dim3(64), 0, c->stream, (const u64 *)c->d_adj, own, (const u64 *)c->d_adj_ref, c->d_asked, c->d_req_flat, c->d_list_n, c->d_req_flat.cap, c->d_ctr);
    ph_end(c, DISCO_PH_CSR);
    HIPCHK(c, hipGetLastError());
    u64 n_flat = 0;
    HIPCHK(c, hipMemcpyAsync(&n_flat, c->d_list_n, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    CHK(read_counters(c));
    if (c->h_ctr[CTR_OVERFLOW]) return fail(c, DISCO_E_CAPACITY, "row requests: list overflow");
    CHK(dist_fetch_rows(c, n_flat));
    c->dinfo.tr_rounds = 1;

    /* marking of the own nodes; nodes beyond the register path or short of a row land in big_list */
    const u64 need_big = nloc + 1024;
    CHK(grow_big_lists(c, need_big));
    HIPCHK(c, hipMemsetAsync(c->d_n_big, 0, sizeof(u32), c->stream));
    c->use_half = true;
    TrArgs a;
    CHK(tr_args_begin(c, &a));
    a.order = c->loci ? c->d_order_own : nullptr; /* (ranks own loci: the own nodes are the list, in the processing order of probe / verify / selection) */
    /* the transitive flags go into the rows of nodes with more than HALF_CAP survivors only, as on one GPU: everybody who judges an edge
     * — the local emission, the survivor push and its receiver — reads a narrow node's survivor LIST and a wide node's row, never a narrow
     * node's row (rounds 1-4 wrote every flag here: a quarter of this kernel's memory requests, left over from the flag exchange the
     * push replaced). DISCO_DIST_ALL_FLAGS=1: as before */
    a.all_flags = getenv("DISCO_DIST_ALL_FLAGS") ? 1u : 0u;
    ph_begin(c, DISCO_PH_TRMARK);
    /* (every node beyond the register path waits for the request-all round here, whatever the LDS arrays could hold: the small variant) */
    if (nloc) wq_launch(c, tr_pick(false, true, true, !a.all_flags), nloc, "DISCO_TR_WAVES", 32, a);
    ph_end(c, DISCO_PH_TRMARK);
    HIPCHK(c, hipGetLastError());
    u32 n_big = 0;
    HIPCHK(c, hipMemcpyAsync(&n_big, c->d_n_big, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    CHK(read_counters(c));
    ph_collect(c);
    if (c->h_ctr[CTR_OVERFLOW]) return fail(c, DISCO_E_CAPACITY, "transitive marking: deferred-node list overflow (%u nodes)", n_big);
    u64 any = n_big;
    CHK(host_reduce(c, &any, 1));
    c->dinfo.tr_deferred = any;
    if (any) { /* round 2 (collective): the listed nodes ask for every row they lack, then take the generic path */
        c->dinfo.tr_rounds = 2;
        u64 bound = 0;
        HIPCHK(c, hipMemsetAsync(c->d_list_n, 0, sizeof(u64), c->stream));
        if (n_big) hipLaunchKernelGGL(list_degree_sum_kernel, dim3(flat_grid(c, n_big)), dim3(256), 0, c->stream, c->d_big_list, (u64)n_big, c->d_adj_ref, c->d_list_n);
        HIPCHK(c, hipMemcpyAsync(&bound, c->d_list_n, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        CHK(ensure(c, c->d_req_flat, bound + 64));
        HIPCHK(c, hipMemsetAsync(c->d_list_n, 0, sizeof(u64), c->stream));
        if (n_big) hipLaunchKernelGGL(tr_request_all_kernel, dim3((int)std::min<u64>(n_big, (u64)c->n_cu * 32)), dim3(64), 0, c->stream, c->d_big_list, (u64)n_big, (const u64 *)c->d_adj, own, (const u64 *)c->d_adj_ref, c->d_asked, c->d_req_flat, c->d_list_n, c->d_req_flat.cap, c->d_ctr);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(&n_flat, c->d_list_n, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
        CHK(read_counters(c));
        if (c->h_ctr[CTR_OVERFLOW]) return fail(c, DISCO_E_CAPACITY, "row requests (round 2): list overflow");
        CHK(dist_fetch_rows(c, n_flat));
        if (n_big) {
            CHK(tr_big_nodes(c, &a, n_big, true, "second round"));
            if (c->h_ctr[CTR_OVERFLOW]) return fail(c, DISCO_E_STATE, "transitive marking: a row was still missing after the request-all round");
        }
    }
    c->n_wide = 0;
    HIPCHK(c, hipMemcpy(&c->n_wide, c->d_n_wide, sizeof(u32), hipMemcpyDeviceToHost));
    c->flags_pending = false;
    c->phase = 7;
    return DISCO_OK;
}

/* ---- 6. surviving half-edges to the owner of the smaller endpoint ---------------------------------------------------- */
static int dist_push_survivors(disco_ctx *c)
{
    DISCO_TRACE("dist_push_survivors");
    const u64 nloc = c->q_hi - c->q_lo;
    const OwnSet own = own_set(c);
    u64 n_items = 0;
    /* the items (survivors whose smaller endpoint is another rank's: 400 000 per rank at 8 x 6.25 M nodes) are written in ONE pass into
     * the room the exchange buffer has anyway (the index records went through it: two per own read) — rounds 1-5 counted them first, a
     * second walk over every own node's survivors and a host round trip. A list that does not fit (the counter of lost items says so)
     * is counted and written again, as before */
    CHK(ensure(c, c->d_x16b, std::max<u64>(nloc / 4, 1u << 16)));
    for (int attempt = 0; attempt < 2; attempt++) {
        u64 cap = attempt ? n_items : c->d_x16b.cap;
        if (!attempt && getenv("DISCO_TEST_TIGHT_PUSH")) cap = std::min<u64>(cap, 1); /* test hook: the first pass loses items, the second one runs */
        HIPCHK(c, hipMemsetAsync(c->d_list_n, 0, sizeof(u64), c->stream));
        CHK(zero_counter(c, CTR_OVERFLOW));
        if (nloc) hipLaunchKernelGGL(emit_push_kernel<true>, dim3(flat_grid(c, nloc, 64)), dim3(64), 0, c->stream, c->d_adj_ref, c->d_adj, c->d_half, c->d_hcnt, c->d_len, own, c->d_x16b, c->d_list_n, cap, c->d_ctr);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(&n_items, c->d_list_n, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
        CHK(read_counters(c)); /* (synchronises: n_items is there) */
        if (!c->h_ctr[CTR_OVERFLOW]) break;
        if (attempt) return fail(c, DISCO_E_STATE, "survivor push: the second pass produced more items than the first counted");
        CHK(ensure(c, c->d_x16b, std::max<u64>(n_items, 1))); /* (the counter counted every item, lost or not) */
    }
    CHK(ensure(c, c->d_x16a, std::max<u64>(n_items, 1)));
    std::vector<u64> scnt, rcnt;
    RouteByNode f{c->per, c->loci ? c->d_otab : nullptr};
    CHK(route_items(c, c->d_x16b.p, n_items, f, c->d_x16a.p, scnt));
    CHK(exchange_counts(c, scnt, rcnt));
    const u64 nr = vsum(rcnt);
    CHK(ensure(c, c->d_x16b, std::max<u64>(nr, 1)));
    CHK(a2a_items(c, DISCO_X_PUSH, c->d_x16a, scnt, c->d_x16b, rcnt, sizeof(ulonglong2)));
    c->d_push_r = c->d_x16b;
    c->n_push_r = nr;
    return DISCO_OK;
}

/* ---- some reads dropped a hit (real data: repeats): complete the lists across ranks, then carry on in the regular regime ------ */
/* Collective. *done = false: too many twins are missing somewhere (or a rank's rows cannot grow in place) — nothing was changed
 * on any rank and the caller gathers the adjacency instead. */
static int dist_complete_twins(disco_ctx *c, bool *done, u64 *asym_total)
{
    DISCO_TRACE("dist_complete_twins");
    const u32 G = (u32)c->comm->world, r = (u32)c->comm->rank;
    const u64 lo = c->q_lo, hi = c->q_hi, nloc = hi - lo, per = c->per;
    const OwnSet own = own_set(c);
    *done = false;
    const auto t0 = HClock::now();
    if (c->loci) {
        /* the reads that dropped something are scattered over the id space (a rank set the bits of ITS reads): their ids travel as
         * lists, every rank sets everybody's bits */
        const u64 n_words = (c->n + 63) / 64;
        u64 mine = 0;
        HIPCHK(c, hipMemsetAsync(c->d_list_n, 0, sizeof(u64), c->stream));
        hipLaunchKernelGGL(bits_to_list_kernel, dim3(flat_grid(c, n_words)), dim3(256), 0, c->stream, (const u64 *)c->d_dropbits, n_words, (u32 *)nullptr, c->d_list_n, (u64)0, c->d_ctr);
        HIPCHK(c, hipMemcpyAsync(&mine, c->d_list_n, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
        std::vector<u64> cnts((size_t)G);
        COMM_CHK(c, c->comm->host_all_gather((const unsigned long long *)&mine, 1, (unsigned long long *)cnts.data(), c->stream)); /* (synchronises: `mine` is there) */
        std::vector<size_t> off((size_t)G), cnt((size_t)G);
        size_t tot = 0;
        for (u32 p2 = 0; p2 < G; p2++) {
            off[p2] = tot * sizeof(u32);
            cnt[p2] = (size_t)cnts[p2] * sizeof(u32);
            tot += (size_t)cnts[p2];
        }
        CHK(ensure(c, c->d_req_flat, std::max<u64>(tot, 1) + 64));
        u32 *my_list = c->d_req_flat + off[r] / sizeof(u32);
        HIPCHK(c, hipMemsetAsync(c->d_list_n, 0, sizeof(u64), c->stream));
        CHK(zero_counter(c, CTR_OVERFLOW));
        hipLaunchKernelGGL(bits_to_list_kernel, dim3(flat_grid(c, n_words)), dim3(256), 0, c->stream, (const u64 *)c->d_dropbits, n_words, my_list, c->d_list_n, (u64)cnts[r], c->d_ctr);
        HIPCHK(c, hipGetLastError());
        COMM_CHK(c, c->comm->all_gather_v(my_list, c->d_req_flat, off.data(), cnt.data(), c->stream));
        if (tot) hipLaunchKernelGGL(list_to_bits_kernel, dim3(flat_grid(c, tot)), dim3(256), 0, c->stream, (const u32 *)c->d_req_flat, (u64)tot, c->d_dropbits);
        HIPCHK(c, hipGetLastError());
        c->dinfo.bytes_sent[DISCO_X_TWINS] += (u64)(G - 1) * cnt[r];
    } else {
        COMM_CHK(c, c->comm->all_gather(c->d_dropbits + (u64)r * per / 64, c->d_dropbits, per / 8, c->stream));
        c->dinfo.bytes_sent[DISCO_X_TWINS] += (u64)(G - 1) * (per / 8);
    }
    c->drop_lo = 0;
    c->drop_hi = c->n;
    /* pairs inside the rank: finds of the own nodes into own nodes that dropped something */
    CHK(twin_check(c, c->loci ? 0 : lo, c->loci ? c->n : hi));
    u64 asym = c->h_ctr[CTR_ASYM];
    /* pairs across ranks: {w, twin} to the owner of w */
    u64 n_items = 0;
    HIPCHK(c, hipMemsetAsync(c->d_list_n, 0, sizeof(u64), c->stream));
    if (nloc) hipLaunchKernelGGL(twin_push_kernel<false>, dim3(flat_grid(c, nloc * 64)), dim3(256), 0, c->stream, c->d_adj_ref, c->d_adj, c->d_len, own, c->d_dropbits,
                                 (ulonglong2 *)nullptr, c->d_list_n, (u64)0, c->d_ctr);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(&n_items, c->d_list_n, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    CHK(ensure(c, c->d_x16b, std::max<u64>(n_items, 1)));
    CHK(ensure(c, c->d_x16a, std::max<u64>(n_items, 1)));
    HIPCHK(c, hipMemsetAsync(c->d_list_n, 0, sizeof(u64), c->stream));
    CHK(zero_counter(c, CTR_OVERFLOW));
    if (nloc) hipLaunchKernelGGL(twin_push_kernel<true>, dim3(flat_grid(c, nloc * 64)), dim3(256), 0, c->stream, c->d_adj_ref, c->d_adj, c->d_len, own, c->d_dropbits,
                                 c->d_x16b, c->d_list_n, n_items, c->d_ctr);
    HIPCHK(c, hipGetLastError());
    CHK(read_counters(c));
    if (c->h_ctr[CTR_OVERFLOW]) return fail(c, DISCO_E_STATE, "twin push: the fill pass produced more items than the count pass");
    std::vector<u64> scnt, rcnt;
    RouteByNode f{per, c->loci ? c->d_otab : nullptr};
    CHK(route_items(c, c->d_x16b.p, n_items, f, c->d_x16a.p, scnt));
    CHK(exchange_counts(c, scnt, rcnt));
    const u64 nr = vsum(rcnt);
    CHK(ensure(c, c->d_x16b, std::max<u64>(nr, 1)));
    CHK(a2a_items(c, DISCO_X_TWINS, c->d_x16a, scnt, c->d_x16b, rcnt, sizeof(ulonglong2)));
    /* room for every received item to turn out missing, behind the extras of the local check */
    const u64 want = (u64)c->n_extra + nr + 1;
    if (want > 0xFFFFFFFFull) return fail(c, DISCO_E_CAPACITY, "twin completion: more than 2^32 extras on one rank");
    if (want > extra_cap(c)) { /* (each keeps its items; a retry after a failure grows the one that is still short) */
        CHK(ensure_keep(c, c->d_extra_node, want, c->n_extra));
        CHK(ensure_keep(c, c->d_extra_key, want, c->n_extra));
    }
    CHK(zero_counter(c, CTR_ASYM));
    CHK(zero_counter(c, CTR_OVERFLOW));
    if (nr) hipLaunchKernelGGL(twin_recv_kernel, dim3(flat_grid(c, nr)), dim3(256), 0, c->stream, (const ulonglong2 *)c->d_x16b, nr, c->d_adj_ref, c->d_adj, c->d_extra_node,
                               c->d_extra_key, c->d_extra_cnt, c->d_n_extra, extra_cap(c), c->d_ctr);
    HIPCHK(c, hipGetLastError());
    u32 ne = 0;
    HIPCHK(c, hipMemcpyAsync(&ne, c->d_n_extra, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    CHK(read_counters(c));
    if (c->h_ctr[CTR_OVERFLOW]) return fail(c, DISCO_E_STATE, "twin completion: extras list overflow");
    asym += c->h_ctr[CTR_ASYM];
    c->n_extra = ne;
    /* can every rank grow its few rows in place? (merge_extras' sparse path; otherwise nothing has been changed yet) */
    u64 need = 0;
    if (ne) {
        HIPCHK(c, hipMemsetAsync(c->d_bump, 0, sizeof(u64), c->stream));
        hipLaunchKernelGGL(merge_need_kernel, dim3(flat_grid(c, c->n)), dim3(256), 0, c->stream, c->d_adj_ref, c->d_extra_cnt, c->n, c->d_bump);
        HIPCHK(c, hipMemcpyAsync(&need, c->d_bump, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    const bool fits = c->d_adj == c->d_hits && ne <= 16384 && c->hits_used + need <= c->d_hits.cap && !getenv("DISCO_MERGE_REBUILD");
    u64 v[2] = {fits ? 0ull : 1ull, asym};
    CHK(host_reduce(c, v, 2));
    c->dinfo.ms[DISCO_X_TWINS] += ms_since(t0);
    *asym_total = v[1];
    if (v[0]) {
        c->n_extra = 0; /* the gathered adjacency is checked again as a whole */
        return DISCO_OK;
    }
    CHK(merge_extras(c));
    *done = true;
    return DISCO_OK;
}

/* every rank's degrees and rows on every rank, imported as the context's adjacency; with them the bitmaps of the reads that dropped a hit */
static int dist_gather_adjacency(disco_ctx *c, const std::vector<u64> &adj_totals, u64 total)
{
    const u32 G = (u32)c->comm->world, r = (u32)c->comm->rank;
    const u64 per = c->per;
    LocalBuf<u32> deg_all(c);
    LocalBuf<u64> rows_all(c);
    CHK(ensure(c, deg_all, (u64)G * per));
    CHK(ensure(c, rows_all, std::max<u64>(total, 1)));
    u64 base = 0;
    for (u32 p = 0; p < r; p++) base += adj_totals[p];
    const auto t0 = HClock::now();
    if (hipMemsetAsync(deg_all + (u64)r * per, 0, per * sizeof(u32), c->stream) != hipSuccess) return DISCO_E_HIP;
    CHK(disco_export_adjacency(c, deg_all + (u64)r * per, rows_all + base));
    CHK(c->comm->all_gather(deg_all + (u64)r * per, deg_all, per * sizeof(u32), c->stream));
    std::vector<size_t> off((size_t)G), cnt((size_t)G);
    size_t a = 0;
    for (u32 p = 0; p < G; p++) {
        off[p] = a;
        cnt[p] = adj_totals[p] * sizeof(u64);
        a += cnt[p];
        if (p != r) c->dinfo.bytes_sent[DISCO_X_ADJACENCY] += cnt[r] + per * sizeof(u32);
    }
    CHK(c->comm->all_gather_v(rows_all + base, rows_all, off.data(), cnt.data(), c->stream));
    if (hipStreamSynchronize(c->stream) != hipSuccess) return DISCO_E_HIP;
    c->dinfo.ms[DISCO_X_ADJACENCY] += ms_since(t0);
    CHK(disco_import_adjacency(c, deg_all, rows_all, total));
    /* which reads dropped a hit (ranges are multiples of 64 reads: whole bitmap words): the twin search below is limited to them */
    CHK(c->comm->all_gather(c->d_dropbits + (u64)r * per / 64, c->d_dropbits, per / 8, c->stream));
    c->dinfo.bytes_sent[DISCO_X_ADJACENCY] += (u64)(G - 1) * (per / 8);
    c->drop_lo = 0;
    c->drop_hi = c->n;
    return DISCO_OK;
}

/* ---- order-dependent regime: everybody gets the whole adjacency and finishes the pass on its own --------------------- */
static int dist_irregular(disco_ctx *c, const std::vector<u64> &adj_totals)
{
    DISCO_TRACE("dist_irregular");
    const u64 lo = c->q_lo, hi = c->q_hi;
    const u64 total = vsum(adj_totals);
    int rc = dist_gather_adjacency(c, adj_totals, total); /* (its buffers are gone before the rows are merged and marked) */
    if (rc != DISCO_OK) return c->err.empty() ? fail(c, rc, "adjacency exchange: %s", c->comm->err.c_str()) : rc;
    CHK(disco_symmetrize(c, 1, nullptr));
    CHK(merge_extras(c));
    c->q_lo = 0;
    c->q_hi = c->n;
    rc = disco_transitive_mark(c);
    c->q_lo = lo;
    c->q_hi = hi;
    CHK(rc);
    c->half_complete = true; /* every node was marked here */
    c->dist_active = false;  /* nothing is pushed: every pair is judged locally */
    c->n_push_r = 0;
    return DISCO_OK;
}

extern "C" {

int disco_comm_unique_id(void *out, size_t cap)
{
    if (!out || cap < DISCO_UNIQUE_ID_BYTES) return DISCO_E_ARG;
    static_assert(sizeof(ncclUniqueId) == DISCO_UNIQUE_ID_BYTES, "unique id size");
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return fail(nullptr, DISCO_E_HIP, "ncclGetUniqueId failed");
    memcpy(out, &id, sizeof id);
    return DISCO_OK;
}

static int comm_attach(disco_ctx *c, DiscoComm *cm, DiscoComm *bulk)
{
    delete c->comm;
    delete c->comm_bulk;
    c->comm = cm;
    c->comm_bulk = bulk;
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, DISCO_E_HIP, "hipSetDevice failed");
    if (!c->bulk_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->bulk_stream, hipStreamNonBlocking));
    if (!c->ev_bulk) HIPCHK(c, hipEventCreateWithFlags(&c->ev_bulk, hipEventDisableTiming));
    return DISCO_OK;
}

int disco_comm_init(disco_ctx *c, const void *unique_id, int nranks, int rank)
{
    if (!c || !unique_id || nranks < 1 || nranks > DIST_MAX_WORLD || rank < 0 || rank >= nranks) return c ? fail(c, DISCO_E_ARG, "disco_comm_init: bad argument") : DISCO_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const bool one_comm = getenv("DISCO_DIST_ONE_COMM") != nullptr; /* (every rank alike) */
    RcclComm *cm = new (std::nothrow) RcclComm();
    RcclComm *bulk = one_comm ? nullptr : new (std::nothrow) RcclComm();
    if (!cm || (!bulk && !one_comm)) {
        delete cm;
        delete bulk;
        return fail(c, DISCO_E_NOMEM, "disco_comm_init: out of host memory");
    }
    /* Order of the steps (round 6): everything that can fail on ONE rank alone — allocations — happens before that rank enters
     * a collective; every decision about the second communicator is taken from values ALL ranks hold (a broadcast, then an all-gather of
     * the ranks' own status), so the ranks keep or drop it together; no rank is ever left waiting inside a collective its peer skipped. */
    int rc = cm->prepare(nranks, rank);                         /* local */
    int bulk_ready = (bulk && bulk->prepare(nranks, rank) == DISCO_OK) ? 1 : 0; /* local; a failure only costs the second communicator */
    if (rc == DISCO_OK) rc = cm->join(unique_id);               /* collective (the launcher's rendezvous: MPI_Init's role) */
    if (rc == DISCO_OK && !one_comm) { /* the id of the second communicator travels over the first one */
        struct IdMsg {
            ncclUniqueId id;
            unsigned long long ok;
        } msg;
        static_assert(sizeof(IdMsg) <= RcclComm::SMALL_VALUES * 8, "fits the staging of host_all_gather");
        memset(&msg, 0, sizeof msg);
        if (rank == 0) msg.ok = ncclGetUniqueId(&msg.id) == ncclSuccess ? 1ull : 0ull;
        void *d_id = cm->d_small;
        memcpy(cm->h_small, &msg, sizeof msg);
        if (hipMemcpyAsync(d_id, cm->h_small, sizeof msg, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            ncclBroadcast(d_id, d_id, sizeof msg, ncclInt8, 0, cm->comm, c->stream) != ncclSuccess ||
            hipMemcpyAsync(cm->h_small, d_id, sizeof msg, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) {
            rc = DISCO_E_HIP; /* the first communicator itself does not work: nothing to fall back to */
            cm->err = "broadcast of the second communicator's id failed";
        } else {
            memcpy(&msg, cm->h_small, sizeof msg);
            /* is everybody able to join it? (rank 0 has an id, every rank its staging) — one all-gather of one word */
            unsigned long long mine = (msg.ok && bulk_ready) ? 1ull : 0ull, all[DIST_MAX_WORLD];
            rc = cm->host_all_gather(&mine, 1, all, c->stream);
            bool everybody = rc == DISCO_OK;
            for (int p = 0; everybody && p < nranks; p++) everybody = all[p] != 0ull;
            if (rc == DISCO_OK && everybody) {
                const int rb = bulk->join(&msg.id); /* collective */
                /* ... and did everybody get in? Keep it or drop it TOGETHER */
                mine = rb == DISCO_OK ? 1ull : 0ull;
                rc = cm->host_all_gather(&mine, 1, all, c->stream);
                for (int p = 0; rc == DISCO_OK && everybody && p < nranks; p++) everybody = all[p] != 0ull;
            }
            if (rc == DISCO_OK && !everybody) {
                if (rank == 0) fprintf(stderr, "[disco] no second communicator on every rank: the reads are gathered on the first one\n");
                delete bulk;
                bulk = nullptr;
            }
        }
    }
    if (one_comm) {
        delete bulk;
        bulk = nullptr;
    }
    if (rc == DISCO_OK && bulk) { /* abort() of either takes both down */
        cm->sibling = bulk;
        bulk->sibling = cm;
    }
    if (rc != DISCO_OK) {
        fail(c, rc, "disco_comm_init: %s %s", cm->err.c_str(), bulk ? bulk->err.c_str() : "");
        delete cm;
        delete bulk;
        return rc;
    }
    return comm_attach(c, cm, bulk);
}

int disco_comm_init_local(disco_ctx *const *ctxs, int nranks)
{
    if (!ctxs || nranks < 1 || nranks > DIST_MAX_WORLD) return DISCO_E_ARG;
    for (int r = 0; r < nranks; r++)
        if (!ctxs[r]) return DISCO_E_ARG;
    auto grp = std::make_shared<LoopGroup>(nranks), grp2 = std::make_shared<LoopGroup>(nranks);
    for (int r = 0; r < nranks; r++) {
        const int rc = comm_attach(ctxs[r], new LoopComm(grp, r), new LoopComm(grp2, r));
        if (rc != DISCO_OK) return rc;
    }
    return DISCO_OK;
}

int disco_probe_run_words(const disco_ctx *c) { return c ? c->runs_lpr : 0; }

/* tests: the processing order the last disco_build_index made (ORDER_MAKE words, n of them) and the reads' grouping keys (by read id) */
int disco_fetch_order(disco_ctx *c, uint64_t *order_words, uint32_t *keys, uint64_t cap, uint64_t *n, int *order_bits)
{
    if (!c || !order_words || !keys || !n || !order_bits) return DISCO_E_ARG;
    if (!c->order_ready || !c->d_order_own || !c->d_okey) return fail(c, DISCO_E_STATE, "disco_fetch_order: disco_build_index made no order");
    *n = c->n;
    *order_bits = c->order_counted_bits;
    if (cap < c->n) return fail(c, DISCO_E_ARG, "disco_fetch_order: room for %llu reads, %llu needed", (unsigned long long)cap, (unsigned long long)c->n);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(order_words, c->d_order_own, c->n * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(keys, c->d_okey, c->n * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DISCO_OK;
}
int disco_fetch_survivor_layout(disco_ctx *c, uint8_t *list_len, uint64_t cap, uint64_t *n, int *dense, uint64_t *out_used)
{
    if (!c || !n || !dense || !out_used) return DISCO_E_ARG;
    if (c->phase < 8) return fail(c, DISCO_E_STATE, "disco_fetch_survivor_layout: run disco_transitive_reduce first");
    *n = c->n;
    *dense = c->out_dense ? 1 : 0;
    *out_used = c->out_used;
    if (!list_len) return DISCO_OK;
    if (cap < c->n) return fail(c, DISCO_E_ARG, "disco_fetch_survivor_layout: room for %llu nodes, %llu needed", (unsigned long long)cap, (unsigned long long)c->n);
    if (!c->half_selfdel || !c->d_half) return fail(c, DISCO_E_STATE, "disco_fetch_survivor_layout: the last marking kept counts, not self-delimiting lists");
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<u64> half(c->n * HALF_CAP), ref(c->n);
    if (c->n) {
        HIPCHK(c, hipMemcpyAsync(half.data(), c->d_half, c->n * HALF_CAP * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(ref.data(), c->d_adj_ref, c->n * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    for (u64 v = 0; v < c->n; v++) /* (a node without a row has no list this pass: whatever an earlier pass left) */
        list_len[v] = REF_DEG(ref[v]) ? (uint8_t)surv_len(half[4 * v], half[4 * v + 1], half[4 * v + 2], half[4 * v + 3]) : 0xFFu;
    return DISCO_OK;
}
int disco_set_order_sub_bits(disco_ctx *c, int bits, int *in_use)
{
    if (!c) return DISCO_E_ARG;
    if (in_use) *in_use = c->order_sub_bits;
    if (bits >= 0) c->order_sub_limit = std::min(bits, ORDER_SUB_MAX);
    return DISCO_OK;
}
int disco_comm_rank(const disco_ctx *c) { return (c && c->comm) ? c->comm->rank : 0; }
int disco_comm_world(const disco_ctx *c) { return (c && c->comm) ? c->comm->world : 1; }
const char *disco_comm_kind(const disco_ctx *c) { return (c && c->comm) ? c->comm->kind() : "none"; }

int disco_dist_range(const disco_ctx *c, uint64_t n_total, uint64_t *lo, uint64_t *hi)
{
    if (!c || !lo || !hi) return DISCO_E_ARG;
    u64 per, l, h;
    dist_range(c, n_total, &per, &l, &h);
    *lo = l;
    *hi = h;
    return DISCO_OK;
}

/* table of world * per rows; the own range is filled by the caller / generator, the rest by the all-gather of the pass */
static int dist_set_reads(disco_ctx *c, u64 n_total, uint32_t dstride)
{
    if (!c->comm) return fail(c, DISCO_E_STATE, "no communicator: call disco_comm_init / disco_comm_init_local first");
    u64 per, lo, hi;
    dist_range(c, n_total, &per, &lo, &hi);
    CHK(begin_rows(c, n_total, per * (u64)c->comm->world, 0, dstride, false));
    c->per = per;
    c->q_lo = c->home_lo = lo;
    c->q_hi = c->home_hi = hi;
    /* unused words of a row are zero (disco_device.h): the other ranks' rows arrive at their used words only */
    HIPCHK(c, hipMemsetAsync(c->d_reads, 0, c->n_alloc * (u64)dstride * 8, c->stream));
    c->dist_reads = true;
    c->ingest_n = 0; /* (disco_dist_ingest_fasta sets it again behind this: only its reads have record numbers to fetch) */
    return DISCO_OK;
}

static int dist_validate(disco_ctx *c)
{
    const u64 nloc = c->q_hi - c->q_lo;
    CHK(count_lengths(c, c->q_lo, c->q_hi));
    /* the job's longest / shortest read (the shortest travels complemented, so both are a maximum over the ranks): every rank
     * then takes the same two-pass decision in disco_probe whatever its own reads or its context's history look like */
    u64 bad = c->h_ctr[CTR_BAD_LEN], ext[2] = {c->h_ctr[CTR_MAX_LEN], c->h_ctr[CTR_MIN_LEN]};
    CHK(host_reduce(c, &bad, 1));
    CHK(host_reduce(c, ext, 2, true));
    if (bad) return fail(c, DISCO_E_ARG, "%llu reads have a length outside (min_overlap=%u, min(32767, 32*stride)]", (unsigned long long)bad, c->prm.min_overlap);
    c->max_len = (u32)ext[0];
    c->min_len = 0xFFFFu - (u32)ext[1];
    /* the k-mer probes of the home range (disco_dist_info.probes): a property of the reads, summed once here instead of in every pass */
    CHK(ensure(c, c->d_list_n, 1));
    HIPCHK(c, hipMemsetAsync(c->d_list_n, 0, sizeof(u64), c->stream));
    if (nloc) hipLaunchKernelGGL(probes_sum_kernel, dim3(flat_grid(c, nloc)), dim3(256), 0, c->stream, c->d_len, c->q_lo, c->q_hi, (u32)c->k, c->d_list_n);
    HIPCHK(c, hipMemcpyAsync(&c->home_probes, c->d_list_n, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    /* round 6: the job's long reads and the longest of the others (two classes of rows under a communicator: every rank decides alike) */
    c->job_n_long = 0;
    c->job_short_max = c->max_len;
    if (c->max_len > (u32)DISCO_SHORT_MAX) {
        LocalBuf<u64> d_ls(c);
        u64 hls[2] = {0, 0};
        CHK(ensure(c, d_ls, 2));
        HIPCHK(c, hipMemsetAsync(d_ls, 0, 2 * sizeof(u64), c->stream));
        if (nloc) hipLaunchKernelGGL(long_stats_kernel, dim3(flat_grid(c, nloc)), dim3(256), 0, c->stream, (const u16 *)c->d_len, c->q_lo, c->q_hi, d_ls);
        HIPCHK(c, hipMemcpyAsync(hls, d_ls, sizeof hls, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        release(c, d_ls); /* (before the ranks meet) */
        CHK(host_reduce(c, &hls[0], 1));
        CHK(host_reduce(c, &hls[1], 1, true));
        c->job_n_long = hls[0];
        c->job_short_max = (u32)hls[1];
    }
    c->phase = 1;
    return DISCO_OK;
}

int disco_dist_upload_reads(disco_ctx *c, const uint64_t *packed_own, uint32_t stride_words, const uint16_t *len_own, uint64_t n_total)
{
    DISCO_TRACE("disco_dist_upload_reads");
    if (!c) return DISCO_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const uint32_t dstride = (stride_words + 7u) & ~7u;
    CHK(dist_set_reads(c, n_total, dstride));
    const u64 nloc = c->q_hi - c->q_lo;
    if (nloc && (!packed_own || !len_own)) return fail(c, DISCO_E_ARG, "disco_dist_upload_reads: null argument");
    if (nloc) {
        u64 *dst = c->d_reads + c->q_lo * (u64)dstride;
        if (dstride != stride_words) HIPCHK(c, hipMemsetAsync(dst, 0, nloc * (u64)dstride * 8, c->stream));
        HIPCHK(c, hipMemcpy2DAsync(dst, (size_t)dstride * 8, packed_own, (size_t)stride_words * 8, (size_t)stride_words * 8, nloc, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->d_len + c->q_lo, len_own, nloc * 2, hipMemcpyHostToDevice, c->stream));
    }
    return dist_validate(c);
}

int disco_dist_generate_reads(disco_ctx *c, const disco_genspec_abi *s)
{
    DISCO_TRACE("disco_dist_generate_reads");
    if (!c || !s) return c ? fail(c, DISCO_E_ARG, "disco_dist_generate_reads: null argument") : DISCO_E_ARG;
    disco_genspec g;
    uint32_t stride = 0;
    CHK(gen_spec(c, "disco_dist_generate_reads", s, &g, &stride));
    HIPCHK(c, hipSetDevice(c->device));
    CHK(dist_set_reads(c, s->n_reads, stride));
    const u64 nloc = c->q_hi - c->q_lo;
    if (nloc) hipLaunchKernelGGL(generate_reads_kernel, dim3(flat_grid(c, nloc * stride)), dim3(256), 0, c->stream, g, c->d_reads, c->d_len, (int)stride, c->q_lo, c->q_hi);
    HIPCHK(c, hipGetLastError());
    return dist_validate(c);
}

/* ---- the device input stage on every rank (include/disco_hip.h: disco_dist_ingest_fasta): the second driver of the input stage's steps
 * ("input stage on the GPU" above; kernels: disco_ingest.h). Particular to it: the byte shares, a pinned ring of the call's own, the
 * tail behind a piece, and the three places where all ranks meet:
 *   A  its pieces into HBM; FASTA: record starts; FASTQ: newlines of the owned bytes
 *      -- all-gather: status word + newlines per (rank, file) --
 *   B  FASTQ: record starts from the line phase; clean + filter of the piece's records
 *      -- all-gather: status word + the per-piece figures --
 *   C  every rank folds the same figures (ingest_fold); table of the job's shape (dist_set_reads); lengths, record numbers and rows of
 *      the share at their global ids
 *      -- all-gather: status word -- all-to-all of rows, lengths, record numbers: what lies outside the home range, to its owner
 *   dist_validate (collective, as behind an upload)
 * A local failure or decline never returns in front of the next meeting point: it travels in the status word, and everybody leaves
 * behind that all-gather with the same code.
 * DISCO_DIST_BGZF=1: a BGZF file is a file whose bytes are those of its TEXT. Every rank walks its member chain in front of the shares
 * (di_walk_bgzf), and in step A a piece's text is decoded from the members that hold it (ingest_piece_text_bgzf) instead of read; from
 * ingest_count_starts on nothing knows the difference. */
extern "C++" {
namespace {
enum { DI_OK = 0, DI_DECLINE = 1, DI_ERROR = 2 };
constexpr u64 DI_TAIL = 1ull << 21; /* bytes behind a piece: the rest of its last record (a longer one declines the file on one GPU too) */

inline u64 di_status(int kind, int code, size_t file) { return ((u64)kind << 60) | ((u64)file << 16) | (u64)code; }

/* n values per rank -> all[world][n], in calls of at most the communicator's staging */
int di_gather(disco_ctx *c, const std::vector<u64> &mine, std::vector<u64> &all)
{
    const size_t G = (size_t)c->comm->world, n = mine.size(), STEP = RcclComm::SMALL_VALUES;
    all.assign(G * n, 0);
    std::vector<u64> part;
    for (size_t at = 0; at < n; at += STEP) {
        const size_t m = std::min(STEP, n - at);
        part.resize(G * m);
        COMM_CHK(c, c->comm->host_all_gather((const unsigned long long *)mine.data() + at, (int)m, (unsigned long long *)part.data(), c->stream));
        for (size_t g = 0; g < G; g++) memcpy(&all[g * n + at], &part[g * m], m * 8);
    }
    return DISCO_OK;
}

struct DistIngest {
    disco_ctx *c;
    IngestJob job;
    void *ring = nullptr;
    size_t ring_bytes = 0;
    u64 status = 0; /* this rank's */
    size_t n_bgzf = 0; /* BGZF files of the job, and what walking their member chains took on this rank */
    float walk_ms = 0;
    DistIngest(disco_ctx *ctx, int n_files, uint32_t threads) : c(ctx), job(ctx, "disco_dist_ingest_fasta", n_files, threads) {}
    ~DistIngest()
    {
        if (ring) (void)hipHostFree(ring);
        release(c, c->d_ingest);
    }
    /* a step's answer into the status word (the first one stays) */
    void note(int rc)
    {
        if (rc == DISCO_OK || status) return;
        status = rc == INGEST_DECLINED ? di_status(DI_DECLINE, job.why_code, job.why_file) : di_status(DI_ERROR, -rc, 0);
    }
};
} // namespace
} // extern "C++"

/* every rank's verdict -> one for all: the error of the lowest rank that has one, else the decline of the lowest file (lowest rank) */
static int di_verdict(DistIngest &D, const std::vector<u64> &all, size_t n_per_rank, const char *const *paths)
{
    disco_ctx *c = D.c;
    const int G = c->comm->world;
    int dec_rank = -1;
    u64 dec = 0;
    for (int g = 0; g < G; g++) {
        const u64 st = all[(size_t)g * n_per_rank];
        const int kind = (int)(st >> 60);
        if (kind == DI_ERROR) {
            const int rc = -(int)(st & 0xFFFFu);
            if (g == c->comm->rank) return rc; /* (its own message stands) */
            return fail(c, rc, "disco_dist_ingest_fasta: rank %d failed (%d) in its share of the input", g, rc);
        }
        if (kind == DI_DECLINE && (dec_rank < 0 || ((st >> 16) & 0xFFFFFFFFull) < ((dec >> 16) & 0xFFFFFFFFull))) {
            dec_rank = g;
            dec = st;
        }
    }
    if (dec_rank < 0) return DISCO_OK;
    const size_t file = (size_t)((dec >> 16) & 0xFFFFFFFFull);
    const int code = (int)(dec & 0xFFFFu);
    c->err.clear();
    /* (which member and why is known to the rank that met it — its DISCO_VERBOSE line says so; the status word carries the code) */
    const char *const more = code == DR_GZ_MEMBER ? " a member chain that does not hold" : (code == DR_BGZF_MEMBER ? ": a member the decoder or its CRC32 refuses" : "");
    return fail(c, DISCO_E_UNSUPPORTED, "disco_dist_ingest_fasta: %s%s (%s; seen by rank %d): the host input stage takes this job", kIngestDecline[code > 0 && code < DR_COUNT ? code : 0], more,
                paths[file] ? paths[file] : "", dec_rank);
}

/* step (every rank, DISCO_DIST_BGZF=1): a BGZF file's member chain, the size of its text and — what every rank must know of a file
 * before it counts anything — its first and its last text byte, from the first and the last member that have text, decoded here on
 * the host by the kernel's own functions and checked as the kernel checks them. Every rank sees the same file: a decline is everybody's */
static int di_walk_bgzf(IngestJob &j, IngestFile &f, float *walk_ms)
{
    const auto t0 = HClock::now();
    uint64_t total = 0, bad = 0;
    const char *why = infl::bgzf_walk(f.map, f.comp_n, f.blocks, &total, &bad);
    *walk_ms += ms_since(t0);
    char msg[160];
    if (why || total == 0) {
        snprintf(msg, sizeof msg, "member %llu: %s", (unsigned long long)bad, why ? why : "no text");
        return j.decline(DR_GZ_MEMBER, f, msg);
    }
    f.n = total;
    size_t k0 = 0, k1 = f.blocks.size() - 1;
    while (f.blocks[k0].isize == 0) k0++;
    while (f.blocks[k1].isize == 0) k1--;
    std::vector<u8> text(INFL_MAX_ISIZE);
    std::unique_ptr<infl::Tables> tab(new infl::Tables);
    char first = 0;
    for (size_t k = k0;; k = k1) { /* (one member with text: decoded once) */
        if (const int e = infl::bgzf_member_host(f.map, f.blocks[k], text.data(), *tab)) {
            snprintf(msg, sizeof msg, "member %llu: %s", (unsigned long long)k, infl::reason(e));
            return j.decline(DR_BGZF_MEMBER, f, msg);
        }
        if (k == k0) first = (char)text[0];
        f.last = (char)text[f.blocks[k].isize - 1];
        if (k == k1) break;
    }
    if (first != '>' && first != '@') return j.decline(DR_FORM, f);
    f.fastq = first == '@';
    return DISCO_OK;
}

/* step: the text of a piece of a BGZF file — the window [p0 - own_lo, pend) of the file's text — out of the members that hold it: their
 * compressed bytes into HBM (ONE range of the file), the table counted from there, one wavefront per member, the first and the last
 * one clipped to the window. Behind it the piece is what ingest_piece_text leaves of a plain file; the byte in front of the owned
 * bytes and their last one are looked at in the decoded text */
static int ingest_piece_text_bgzf(IngestJob &j, IngestFile &f, void *ring, size_t ring_bytes)
{
    disco_ctx *c = j.c;
    IngestPiece &p = f.p;
    const auto t_read = HClock::now();
    std::vector<infl::BgzfBlock> sub;
    uint64_t comp_lo = 0, comp_n = 0, bad = 0;
    infl::bgzf_rebase(f.blocks, f.m_first, f.m_count, sub, &comp_lo, &comp_n);
    if (sub.empty()) return fail(c, DISCO_E_STATE, "disco_dist_ingest_fasta: a piece of %s without a member", f.path.c_str());
    infl::BgzfBlock *d_blk = nullptr;
    u32 *d_status = nullptr;
    CHK(j.get(&p.d_text, ingest_text_cap(p.n)));
    CHK(j.get(&f.d_comp, comp_n));
    CHK(j.get(&d_blk, sub.size()));
    CHK(j.get(&d_status, sub.size() + 1));
    HIPCHK(c, hipMemsetAsync(p.d_text + p.n, 0, ingest_text_cap(p.n) - p.n, c->stream));
    const int rc = ingest_read_file(c, f.fd, comp_n, f.d_comp, j.threads, comp_lo, ring, ring_bytes);
    j.read_s += ms_since(t_read) * 1e-3f;
    CHK(rc);
    int e = infl::INFL_OK;
    CHK(bgzf_inflate_run(c, f.d_comp, sub.data(), sub.size(), d_blk, d_status, p.d_text, p.p0 - p.own_lo, p.n, &bad, &e));
    if (e != infl::INFL_OK) {
        char msg[160];
        snprintf(msg, sizeof msg, "member %llu: %s", (unsigned long long)(f.m_first + bad), infl::reason(e));
        return j.decline(DR_BGZF_MEMBER, f, msg);
    }
    char ch[2] = {'\n', 0};
    if (p.own_lo) HIPCHK(c, hipMemcpy(&ch[0], p.d_text, 1, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(&ch[1], p.d_text + p.own_hi - 1, 1, hipMemcpyDeviceToHost));
    p.prefix_nl = ch[0] == '\n';
    p.last_nl = ch[1] == '\n';
    return DISCO_OK;
}

/* step A, local: the files, the rank's pieces of them, their text in HBM, FASTA record starts / FASTQ newline counts */
static int di_read_pieces(DistIngest &D, const char *const *paths, disco_dist_ingest_info *info)
{
    disco_ctx *c = D.c;
    IngestJob &j = D.job;
    const u64 G = (u64)c->comm->world, r = (u64)c->comm->rank;
    u64 T = 0;
    /* DISCO_DIST_BGZF=1: a .gz name is opened as one GPU opens it, and a BGZF file is T bytes of TEXT like any other: shares, pieces and
     * tails are cut over text bytes. Without it every .gz name declines (DR_GZ_COMM), on this rank and so on all */
    const bool may_bgzf = env_int("DISCO_DIST_BGZF", 0) == 1;
    for (size_t fi = 0; fi < j.F.size(); fi++) {
        IngestFile &f = j.F[fi];
        if (const int code = ingest_open_file(f, paths[fi], may_bgzf)) return j.decline(code == DR_NO_OPEN ? DR_UNREADABLE : code, f);
        if (f.map) {
            if (const int rc = di_walk_bgzf(j, f, &D.walk_ms)) return rc;
            D.n_bgzf++;
        }
        T += f.n;
    }
    /* the rank's share: bytes [a, b) of the files laid end to end
     * (128-bit product: T * r does not fit 64 bits for nothing anybody has, but the cut must be the same arithmetic everywhere) */
    const u64 a = (u64)((unsigned __int128)T * r / G), b = (u64)((unsigned __int128)T * (r + 1) / G);
    info->share_lo = a;
    info->share_hi = b;
    u64 cum = 0, text_bytes = 0;
    for (IngestFile &f : j.F) {
        IngestPiece &p = f.p;
        p.p0 = std::min(std::max(a, cum) - cum, f.n);
        p.p1 = std::min(std::max(b, cum) - cum, f.n);
        cum += f.n;
        if (p.p1 <= p.p0) continue;
        const u64 pend = std::min(f.n, p.p1 + DI_TAIL);
        p.to_eof = pend == f.n;
        p.own_lo = p.p0 ? 1 : 0; /* the byte in front of the piece travels with it; the top of a file has none (the kernels count one: a newline) */
        p.own_hi = p.own_lo + (p.p1 - p.p0);
        p.n = p.own_lo + (pend - p.p0);
        text_bytes += ingest_text_cap(p.n);
        if (f.map) { /* the members that hold the piece: their compressed bytes and their table lie in the arena next to its text */
            infl::bgzf_window_members(f.blocks, p.p0 - p.own_lo, p.n, &f.m_first, &f.m_count);
            const infl::BgzfBlock &m0 = f.blocks[f.m_first], &m1 = f.blocks[f.m_first + f.m_count - 1];
            text_bytes += ((m1.in_off + m1.in_len - m0.in_off + 255) & ~255ull) + ((f.m_count * sizeof(infl::BgzfBlock) + 255) & ~255ull) + (((f.m_count + 1) * 4 + 255) & ~255ull);
            continue; /* (the byte in front and the last owned one: read in the decoded text) */
        }
        char ch[2] = {'\n', 0};
        if ((p.p0 && pread(f.fd, &ch[0], 1, (off_t)(p.p0 - 1)) != 1) || pread(f.fd, &ch[1], 1, (off_t)(p.p1 - 1)) != 1) return fail(c, DISCO_E_ARG, "disco_dist_ingest_fasta: read error");
        p.prefix_nl = ch[0] == '\n';
        p.last_nl = ch[1] == '\n';
    }
    /* the arena and the pinned ring: sized for the SHARE (text + record arrays, a record per 100 bytes at worst here; more: pieces of their own) */
    const u64 own_bytes = text_bytes + (text_bytes / 100) * 28 + (8ull << 20);
    CHK(ensure(c, c->d_ingest, own_bytes));
    j.arena = c->d_ingest.p;
    j.arena_cap = c->d_ingest.cap;
    D.ring_bytes = (size_t)std::min<u64>(256ull << 20, std::max<u64>(1ull << 20, (text_bytes + (1ull << 20) - 1) & ~((1ull << 20) - 1)));
    if (hipHostMalloc(&D.ring, D.ring_bytes, ring_alloc_flags()) != hipSuccess) {
        D.ring = nullptr;
        (void)hipGetLastError();
        return fail(c, DISCO_E_NOMEM, "disco_dist_ingest_fasta: no pinned staging memory");
    }
    for (IngestFile &f : j.F) {
        if (f.p.p1 <= f.p.p0) continue;
        if (f.map) {
            if (const int rc = ingest_piece_text_bgzf(j, f, D.ring, D.ring_bytes)) return rc;
        } else
            CHK(ingest_piece_text(j, f, D.ring, D.ring_bytes));
        CHK(ingest_count_starts(j, f));
    }
    return DISCO_OK;
}

/* step B, local: FASTQ record starts from the exchanged newline counts nl[rank][1 + file]; clean + filter of every piece's records */
static int di_filter_pieces(DistIngest &D, const std::vector<u64> &nl, size_t per_rank)
{
    IngestJob &j = D.job;
    const size_t r = (size_t)D.c->comm->rank;
    for (size_t fi = 0; fi < j.F.size(); fi++) {
        IngestFile &f = j.F[fi];
        if (f.p.p1 <= f.p.p0) continue;
        if (f.fastq) {
            u64 line0 = 0; /* newlines of the file in front of the piece */
            for (size_t g = 0; g < r; g++) line0 += nl[g * per_rank + 1 + fi];
            CHK(ingest_place_starts(j, f, line0));
        }
        CHK(ingest_filter_piece(j, f));
    }
    return DISCO_OK;
}

/* step C, local: the job's table; lengths, record numbers (within the file) and rows of the share at their global ids */
static int di_fill_table(DistIngest &D, const IngestFold &o)
{
    disco_ctx *c = D.c;
    CHK(dist_set_reads(c, o.shape.n, o.shape.stride));
    CHK(ensure(c, c->d_rec_of_read, c->n_alloc));
    CHK(ingest_place_reads(D.job, o));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DISCO_OK;
}

/* what a rank made for ids outside its home range, to the owners: ids [share[g], share[g + 1]) are rank g's, homes are [q per, (q + 1) per).
 * Sender and receiver keep a read at the same row of their tables, so both sides of the all-to-all are the table itself. */
static int di_exchange(disco_ctx *c, const std::vector<u64> &share, void *table, size_t elem)
{
    const int G = c->comm->world, r = c->comm->rank;
    std::vector<size_t> so((size_t)G, 0), sc((size_t)G, 0), ro((size_t)G, 0), rc((size_t)G, 0);
    auto cut = [&](int from, int to, size_t *off, size_t *cnt) { /* ids of rank `from`'s share in rank `to`'s home range */
        const u64 lo = std::max(share[(size_t)from], (u64)to * c->per), hi = std::min(share[(size_t)from + 1], ((u64)to + 1) * c->per);
        *off = hi > lo ? (size_t)lo * elem : 0;
        *cnt = hi > lo ? (size_t)(hi - lo) * elem : 0;
    };
    for (int p = 0; p < G; p++) {
        if (p == r) continue;
        cut(r, p, &so[(size_t)p], &sc[(size_t)p]);
        cut(p, r, &ro[(size_t)p], &rc[(size_t)p]);
    }
    COMM_CHK(c, c->comm->all_to_all_v(table, so.data(), sc.data(), table, ro.data(), rc.data(), c->stream));
    return DISCO_OK;
}

int disco_dist_ingest_fasta(disco_ctx *c, const char *const *paths, int n_files, uint32_t host_threads, disco_dist_ingest_info *info, disco_ingest_file *files)
{
    DISCO_TRACE("disco_dist_ingest_fasta");
    if (!c || !paths || n_files < 1 || !info || !files) return c ? fail(c, DISCO_E_ARG, "disco_dist_ingest_fasta: null argument") : DISCO_E_ARG;
    if (!c->comm) return fail(c, DISCO_E_STATE, "disco_dist_ingest_fasta: no communicator (one GPU: disco_ingest_fasta)");
    const size_t F = (size_t)n_files, G = (size_t)c->comm->world, r = (size_t)c->comm->rank;
    memset(info, 0, sizeof *info);
    info->world = (uint32_t)G;
    DistIngest D(c, n_files, host_threads);
    IngestJob &j = D.job;
    std::vector<u64> mine, all;
    /* A */
    int rc = hipSetDevice(c->device) == hipSuccess ? DISCO_OK : fail(c, DISCO_E_HIP, "hipSetDevice failed");
    if (rc == DISCO_OK) {
        if (c->phase > 1) c->phase = 1;
        rc = di_read_pieces(D, paths, info);
    }
    /* (which member of a BGZF file, and why: the status word has no room for it) */
    if (rc == INGEST_DECLINED && (j.why_code == DR_GZ_MEMBER || j.why_code == DR_BGZF_MEMBER) && getenv("DISCO_VERBOSE")) fprintf(stderr, "[disco] rank %zu declines: %s (%s)\n", r, j.why.c_str(), j.where.c_str());
    D.note(rc);
    mine.assign(1 + F, 0);
    mine[0] = D.status;
    for (size_t fi = 0; fi < F; fi++) mine[1 + fi] = j.F[fi].p.own_nl;
    CHK(di_gather(c, mine, all));
    CHK(di_verdict(D, all, 1 + F, paths));
    /* B */
    D.note(di_filter_pieces(D, all, 1 + F));
    const float t_filtered = j.seconds();
    mine = ingest_figures(j, D.status);
    CHK(di_gather(c, mine, all));
    CHK(di_verdict(D, all, mine.size(), paths));
    /* C: from here on every rank computes the same figures from the same numbers, a decline among them */
    IngestFold o;
    if (ingest_fold(j, all, G, r, files, &o) == INGEST_DECLINED) {
        c->err.clear();
        return fail(c, DISCO_E_UNSUPPORTED, "disco_dist_ingest_fasta: %s (%s): the host input stage takes this job", j.why.c_str(), j.where.c_str());
    }
    const ReadShape &s = o.shape;
    D.status = 0;
    D.note(di_fill_table(D, o));
    mine.assign(1, D.status);
    CHK(di_gather(c, mine, all));
    CHK(di_verdict(D, all, 1, paths));
    CHK(di_exchange(c, o.share, c->d_reads, (size_t)c->S * 8));
    CHK(di_exchange(c, o.share, c->d_len, sizeof(u16)));
    CHK(di_exchange(c, o.share, c->d_rec_of_read.p, sizeof(u32)));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->ingest_n = s.n;
    c->h_len_ok = false;
    info->n_reads = s.n;
    info->total_records = o.total_records;
    info->too_long = o.too_long;
    info->stride_words = std::max<u32>(1, (s.longest + 31) / 32);
    info->shortest = s.shortest;
    info->longest = s.longest;
    info->share_reads = o.share[r + 1] - o.share[r];
    info->home_lo = c->home_lo;
    info->home_hi = c->home_hi;
    {
        const u64 lo = std::max(o.share[r], c->home_lo), hi = std::min(o.share[r + 1], c->home_hi);
        info->kept_reads = hi > lo ? hi - lo : 0;
    }
    const int vrc = dist_validate(c);
    info->read_s = j.read_s;
    info->device_s = j.seconds() - j.read_s;
    if (getenv("DISCO_VERBOSE")) {
        char bgzf[96] = "";
        if (D.n_bgzf) snprintf(bgzf, sizeof bgzf, "; %zu BGZF files, member chains walked in %.1f ms", D.n_bgzf, D.walk_ms);
        fprintf(stderr, "[disco] input stage on rank %zu of %zu: bytes [%llu, %llu) of the input, %llu reads of %llu, %llu kept at home; files %.3f s, records + filter %.3f s, "
                        "table + rows + exchange %.3f s%s\n",
                r, G, (unsigned long long)info->share_lo, (unsigned long long)info->share_hi, (unsigned long long)info->share_reads, (unsigned long long)s.n,
                (unsigned long long)info->kept_reads, j.read_s, t_filtered - j.read_s, j.seconds() - t_filtered, bgzf);
    }
    return vrc;
}

int disco_dist_ingest_fetch(disco_ctx *c, uint16_t *len, uint64_t *file_index)
{
    if (!c || !len || !file_index) return c ? fail(c, DISCO_E_ARG, "disco_dist_ingest_fetch: null argument") : DISCO_E_ARG;
    if (!c->comm || !c->dist_reads || c->phase < 1 || c->ingest_n == 0 || c->ingest_n != c->n)
        return fail(c, DISCO_E_STATE, "disco_dist_ingest_fetch: the reads of the context did not come from disco_dist_ingest_fasta");
    HIPCHK(c, hipSetDevice(c->device));
    return ingest_fetch_range(c, c->home_lo, c->home_hi, c->stream, len, file_index);
}

static int dist_run_graph_pass(disco_ctx *c, uint32_t flags, bool allow_loci, bool *retry_with_id_ranges);

/* one pass; ranks own loci wherever the pass supports it — exact overlaps, fewer than 2^30 reads, the index replicated after its
 * partitioned build (DISCO_DIST_ID_RANGES=1, every rank alike: the id ranges of rounds 1-4). A pass that ends up in the
 * order-dependent regime (the whole adjacency to everybody: too many one-sided pairs) is redone over id ranges: the decision is taken
 * from all-gathered numbers, so every rank takes it alike. */
static int dist_run_graph_impl(disco_ctx *c, uint32_t flags)
{
    bool retry = false;
    int rc = dist_run_graph_pass(c, flags, true, &retry);
    if (rc == DISCO_OK && retry) rc = dist_run_graph_pass(c, flags & ~(uint32_t)DISCO_DIST_GATHER_READS, false, &retry); /* (the reads are everywhere by now) */
    return rc;
}

int disco_dist_run_graph(disco_ctx *c, uint32_t flags)
{
    if (c && c->comm)
        c->time_exchanges = getenv("DISCO_DIST_TIME_EXCHANGES") != nullptr ||
                            (c->dist_passes == 0 && c->comm->world > 1 && !strcmp(c->comm->kind(), "rccl") && !getenv("DISCO_DIST_NO_FIRST_CONTACT"));
    const int rc = dist_run_graph_impl(c, flags);
    if (c) c->dist_passes++;
    if (rc != DISCO_OK && c && c->comm && rc != DISCO_E_ARG && rc != DISCO_E_STATE) {
        /* this rank leaves the pass early: whoever waits for it inside a collective must not wait forever */
        c->comm->abort();
        if (c->comm_bulk) c->comm_bulk->abort();
    }
    return rc;
}

/* the arena of a multi-GPU context (DevArena): made once, before the first collective of the first pass. Sized for what a pass keeps
 * per read — measured with 8 ranks at 50 M x 150 bp (8.9 GB per rank): about 760 bytes per own read (hit buffer, adjacency, headers,
 * exchange buffers) + 46 per read of the job (index, containment keys, bitmaps) — with 60 % on top; DISCO_DIST_ARENA_MB overrides, DISCO_DIST_NO_ARENA=1
 * switches it off (every request then goes to the runtime, as in rounds 1-3) */
static int arena_reserve(disco_ctx *c)
{
    if (c->arena.base || getenv("DISCO_DIST_NO_ARENA")) return DISCO_OK;
    const u64 own = c->q_hi - c->q_lo;
    size_t want = (size_t)((double)(own * 760ull + c->n * 46ull) * 1.6) + (256ull << 20);
    if (const char *e = getenv("DISCO_DIST_ARENA_MB")) want = (size_t)atoll(e) << 20;
    size_t fr = 0, tot = 0;
    HIPCHK(c, hipMemGetInfo(&fr, &tot));
    want = std::min(want, fr / 10 * 9);
    void *p = nullptr;
    while (want >= (64ull << 20)) {
        if (hipMalloc(&p, want) == hipSuccess) break;
        (void)hipGetLastError();
        p = nullptr;
        want /= 2;
    }
    if (!p) return DISCO_OK; /* no arena: the runtime serves the pass (counted) */
    c->arena.base = (char *)p;
    c->arena.size = want & ~(size_t)255;
    c->arena.free_at[0] = c->arena.size;
    return DISCO_OK;
}

static int dist_run_graph_pass(disco_ctx *c, uint32_t flags, bool allow_loci, bool *retry_with_id_ranges)
{
    DISCO_TRACE("disco_dist_run_graph");
    *retry_with_id_ranges = false;
    if (!c) return DISCO_E_ARG;
    if (!c->comm) return fail(c, DISCO_E_STATE, "disco_dist_run_graph: no communicator");
    if (!c->dist_reads || c->phase < 1) return fail(c, DISCO_E_STATE, "disco_dist_run_graph: set the reads with disco_dist_upload_reads / disco_dist_generate_reads");
    HIPCHK(c, hipSetDevice(c->device));
    const u32 G = (u32)c->comm->world, r = (u32)c->comm->rank;
    /* the pass starts from the rank's home range; inside a pass whose ranks own loci q_lo / q_hi are positions of the own list, and
     * whichever way the pass ends they name the home range again */
    struct HomeRange {
        disco_ctx *c;
        ~HomeRange()
        {
            c->q_lo = c->home_lo;
            c->q_hi = c->home_hi;
        }
    } home_range{c};
    c->q_lo = c->home_lo;
    c->q_hi = c->home_hi;
    c->loci = false;
    CHK(arena_reserve(c));
    struct PassToken { /* (in-process transport, DISCO_LOOP_SERIALIZE: one rank's compute segment on the device at a time) */
        DiscoComm *cm;
        explicit PassToken(DiscoComm *x) : cm(x) { cm->begin_pass(); }
        ~PassToken() { cm->end_pass(); }
    } pass_token(c->comm);
    const auto t_pass = HClock::now();
    const PassCounters pc0 = tl_pass;
    const u32 ops0 = c->comm->n_ops + (c->comm_bulk ? c->comm_bulk->n_ops : 0u);
    const u32 hops0 = c->comm->n_host_ops + (c->comm_bulk ? c->comm_bulk->n_host_ops : 0u);
    c->hbm_peak = c->hbm_bytes;
    disco_dist_info &di = c->dinfo;
    memset(&di, 0, sizeof di);
    di.world = G;
    di.rank = r;
    di.n_reads = c->n;
    di.own_lo = c->home_lo;
    di.own_hi = c->home_hi;
    di.own_reads = c->home_hi - c->home_lo;
    c->dist_active = true;
    c->part_index = (flags & DISCO_DIST_KEEP_INDEX_PARTITIONED) != 0 || getenv("DISCO_DIST_PARTITIONED_INDEX") != nullptr;
    /* Round 6 — two classes of rows under a communicator (the reference packs every read at its own length,
     * BG/HashTable.cpp:456-477): a job whose table is wider than 64 bytes because of a FEW long reads (buildG --gpus N on a set with one
     * 600 bp read used to pay the generic probe and the wide-row verify for everybody: 1.6 x) gets 64-byte rows on every rank — each rank
     * converts its replica once the gather of the reads is through (two_class_convert: one pass over the table; the same decision on
     * every rank, from the same table), the pass runs over id ranges (the own reads' index pass needs the converted table, i.e. the whole
     * gather: nothing is dealt ahead), the long reads of a rank's range take the long class's kernels as on one GPU. Every rank decides
     * alike: the shape of the JOB (stride, longest read: dist_validate reduced them). DISCO_DIST_NO_TWO_CLASS=1: one stride, as before. */
    bool ragged_job = false;
    if (!c->part_index && c->prm.max_substitutions == 0 && !getenv("DISCO_DIST_NO_TWO_CLASS") && !getenv("DISCO_NO_TWO_CLASS")) {
        if (c->two_class) ragged_job = true;
        else if (c->S > VERIFY_SW && c->job_n_long) { /* the test of a single GPU (at most one long read in five, run lists for the others), on the JOB's figures */
            c->dist_two_class = true;
            ragged_job = two_class_ok(c, c->S, c->n, c->job_n_long, c->job_short_max);
            c->dist_two_class = false;
        }
    }
    const bool want_loci = allow_loci && !ragged_job && !c->part_index && c->prm.max_substitutions == 0 && c->n < (1ull << 30) && !getenv("DISCO_DIST_ID_RANGES") && !getenv("DISCO_DIST_FORCE_GATHER");
    c->n_push_r = 0;
    c->h_len.clear();
    /* 0. everybody gets every read — on the second communicator and stream: the index build and the probe of the own reads
     *    need nothing of it, verify waits for it (disco_probe).
     *    Two communicators in flight on one device are safe when every rank issues their operations in the same order (RCCL / NCCL's
     *    rule for concurrent communicators) and every kernel that shares the device with them terminates: all ranks run this very
     *    function — the all-gather of the reads is the only kind of operation comm_bulk ever carries and sits at the same place of
     *    the program order of every rank, in front of the pass's operations on comm — and the compute kernels next to it are finite passes over a work
     *    queue. DISCO_DIST_ONE_COMM=1 (every rank alike) takes the second communicator out of the picture: the all-gather then runs on
     *    comm and the context's stream, in front of the index exchanges, at the price of its 5 ms (G = 8, config 4) on the critical path. */
    const bool one_comm = c->comm_bulk == nullptr || getenv("DISCO_DIST_ONE_COMM") != nullptr;
    DiscoComm *const bulk = one_comm ? c->comm : c->comm_bulk;
    const hipStream_t bstream = one_comm ? c->stream : c->bulk_stream;
    if ((flags & DISCO_DIST_GATHER_READS) && !c->two_class) { /* (a table that has its two classes is complete: an earlier pass gathered it) */
        const auto t0 = HClock::now();
        const u64 row_bytes = (u64)c->S * 8;
        HIPCHK(c, hipStreamSynchronize(c->stream)); /* the own rows are in place */
#define BULK_CHK(expr)                                                                                        \
    do {                                                                                                      \
        int rc_ = (expr);                                                                                     \
        if (rc_ != DISCO_OK) return fail(c, rc_, "%s: %s", #expr, bulk->err.c_str());                 \
    } while (0)
        const int W = (int)((c->max_len + 31) / 32); /* words the longest read of the job uses (150 bp: 5 of the 8-word stride) */
        u64 sent_row_bytes = row_bytes;
        if (W < c->S && !getenv("DISCO_DIST_FULL_ROWS")) {
            /* pack the own rows, all-gather the dense array, spread the other ranks' rows back over the table: 37 % fewer bytes
             * on the links at 150 bp, paid with two streaming passes on the second stream while the index is being built */
            /* a rank's block = its rows and, behind them, its lengths (per is a multiple of 64: 2 per bytes are whole words): ONE operation */
            const u64 total_rows = c->per * (u64)G;
            const u64 rows_words = c->per * (u64)W, block_words = rows_words + c->per / 4;
            CHK(ensure(c, c->d_dense, block_words * (u64)G));
            u64 *mine = c->d_dense + (u64)r * block_words;
            hipLaunchKernelGGL(pack_rows_kernel, dim3(flat_grid(c, c->per * W)), dim3(256), 0, bstream, c->d_reads, c->S, W, (u64)r * c->per, c->per, mine);
            HIPCHK(c, hipMemcpyAsync(mine + rows_words, c->d_len + (u64)r * c->per, c->per * 2, hipMemcpyDeviceToDevice, bstream));
            BULK_CHK(bulk->all_gather(mine, c->d_dense, block_words * 8, bstream));
            hipLaunchKernelGGL(unpack_rows_kernel, dim3(flat_grid(c, total_rows * W)), dim3(256), 0, bstream, c->d_dense, c->S, W, total_rows, (u64)r * c->per,
                               (u64)(r + 1) * c->per, c->d_reads, c->per, block_words);
            hipLaunchKernelGGL(unpack_lens_kernel, dim3(flat_grid(c, total_rows)), dim3(256), 0, bstream, (const u64 *)c->d_dense, c->per, block_words, rows_words, G, r, c->d_len);
            HIPCHK(c, hipGetLastError());
            sent_row_bytes = (u64)W * 8;
        } else {
            BULK_CHK(bulk->all_gather(c->d_reads + (u64)r * c->per * c->S, c->d_reads, c->per * row_bytes, bstream));
            BULK_CHK(bulk->all_gather(c->d_len + (u64)r * c->per, c->d_len, c->per * 2, bstream));
        }
#undef BULK_CHK
        HIPCHK(c, hipEventRecord(c->ev_bulk, bstream));
        c->wait_bulk_before_verify = true;
        di.bytes_sent[DISCO_X_READS] += (u64)(G - 1) * c->per * (sent_row_bytes + 2);
        di.ms[DISCO_X_READS] += ms_since(t0); /* time to ISSUE it (RCCL: asynchronous; in-process transport: the copies themselves) */
    }
    if (ragged_job && !c->two_class) {
        if (c->wait_bulk_before_verify) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_bulk, 0)); /* the whole table, then its two classes */
        c->dist_two_class = true;
        const int rc2 = two_class_convert(c);
        c->dist_two_class = false;
        CHK(rc2);
    }
    if (want_loci) CHK(dist_deal_reads(c));
    di.placement = c->loci ? 1u : 0u;
    CHK(dist_build_index(c));
    c->contained_done = false;
    CHK(disco_probe(c));
    if (!c->contained_done) CHK(dist_mark_contained(c));
    CHK(select_edges(c));
    /* whole-job figures and the regime decision */
    const u64 probes = c->home_probes; /* (dist_validate) */
    CHK(ensure(c, c->d_list_n, 1));
    u64 g[8] = {c->adj_total, c->dropped_local, c->n_contained, c->h_ctr[CTR_CAP_SITES], c->h_ctr[CTR_KMER_HITS], probes, 0, 0};
    {
        constexpr int NV = 6;
        std::vector<u64> all((size_t)G * NV);
        COMM_CHK(c, c->comm->host_all_gather((const unsigned long long *)g, NV, (unsigned long long *)all.data(), c->stream));
        std::vector<u64> adj_totals((size_t)G);
        u64 sum[NV] = {0, 0, 0, 0, 0, 0};
        for (u32 p = 0; p < G; p++) {
            adj_totals[p] = all[(size_t)p * NV];
            for (int i = 0; i < NV; i++) sum[i] += all[(size_t)p * NV + i];
        }
        di.probes = sum[5];
        di.dropped_hits = sum[1];
        di.n_contained = sum[2];
        di.n_contained_local = c->n_contained;
        di.cap_bind_sites = sum[3];
        di.kmer_hits = sum[4];
        di.e_pre = sum[0] / 2;
        c->dropped = sum[1];
        bool irregular = c->n >= (1ull << 30) || c->prm.max_substitutions != 0 || getenv("DISCO_DIST_FORCE_GATHER");
        u64 asym_total = 0;
        if (!irregular && sum[1] != 0) {
            /* somebody dropped a hit (per-k-mer cap, second hit to a destination: real data do at their repeats). Only the lists of
             * the reads that dropped something can lack a twin: complete those across ranks, then the regular regime applies */
            bool done = false;
            if (!getenv("DISCO_DIST_NO_TWIN_PUSH")) CHK(dist_complete_twins(c, &done, &asym_total));
            irregular = !done;
            if (done) {
                u64 t[1] = {c->adj_total};
                CHK(host_reduce(c, t, 1));
                di.e_pre = t[0] / 2;
                di.regime = 2;
            }
        }
        if (irregular && c->loci) { /* the gather of the whole adjacency walks id ranges: the pass is redone over them (collective decision) */
            *retry_with_id_ranges = true;
            c->loci = false;
            return DISCO_OK;
        }
        if (irregular) {
            di.regime = 1;
            CHK(dist_irregular(c, adj_totals));
            di.e_pre = c->adj_total / 2;
            di.asymmetric_pairs = c->asym_local;
        } else {
            c->phase = 6; /* nobody dropped a hit, or the lists have just been completed: they are symmetric (twin_check's argument) */
            c->n_extra = 0;
            c->asym_local = asym_total;
            di.asymmetric_pairs = asym_total;
            if (di.regime == 0) c->ph_ms[DISCO_PH_TWIN] = 0;
            CHK(dist_transitive_mark(c));
            CHK(dist_push_survivors(c));
        }
    }
    uint64_t n_out = 0;
    CHK(disco_emit_edges(c, &n_out));
    CHK(settle_keys(c)); /* (whatever reads best[] after the pass — disco_fetch_contained — runs on this stream, behind the keys) */
    u64 tot[1] = {(u64)n_out};
    CHK(host_reduce(c, tot, 1));
    di.e_out = tot[0];
    di.e_out_local = n_out;
    di.ms_total = ms_since(t_pass);
    di.device_allocs = tl_pass.dev_allocs - pc0.dev_allocs;
    di.device_frees = tl_pass.dev_frees - pc0.dev_frees;
    di.host_syncs = tl_pass.host_syncs - pc0.host_syncs + (c->comm->n_host_ops + (c->comm_bulk ? c->comm_bulk->n_host_ops : 0u) - hops0);
    di.comm_ops = c->comm->n_ops + (c->comm_bulk ? c->comm_bulk->n_ops : 0u) - ops0;
    di.arena_bytes = c->arena.size;
    di.arena_peak = c->arena.peak;
    di.hbm_peak = c->hbm_peak;
    {
        float km = 0;
        for (int i = 0; i < DISCO_PH_COUNT; i++) km += c->ph_ms[i];
        di.kernel_ms = km;
    }
    return DISCO_OK;
}

int disco_dist_get_info(disco_ctx *c, disco_dist_info *out)
{
    if (!c || !out) return DISCO_E_ARG;
    *out = c->dinfo;
    return DISCO_OK;
}

/* ---- the text files of a multi-GPU job, every rank its own (disco_text.h) -------------------------------------------------------------
 * For F files of one kind and G ranks, rank r writes the files f with floor(f G / F) == r: the run [ceil(r F / G), ceil((r + 1) F / G)),
 * empty for some ranks when F < G. */
static void dist_own_files(const disco_ctx *c, uint32_t n_files, uint32_t *f_lo, uint32_t *f_hi)
{
    const u64 G = (u64)c->comm->world, r = (u64)c->comm->rank, F = n_files;
    *f_lo = (uint32_t)((r * F + G - 1) / G);
    *f_hi = (uint32_t)(((r + 1) * F + G - 1) / G);
}

/* what a rank did on its own between two collectives, agreed on: DISCO_OK when every rank says so, else the rank's own code or the
 * first failing peer's — the ranks leave a collective entry point alike, and the caller's next collective is entered by all or by none */
static int dist_agree(disco_ctx *c, const char *who, int rc)
{
    const size_t G = (size_t)c->comm->world;
    std::vector<u64> st(G);
    const u64 mine = (u64)(int64_t)rc;
    const std::string own = rc != DISCO_OK ? c->err : std::string();
    const int xrc = c->comm->host_all_gather((const unsigned long long *)&mine, 1, (unsigned long long *)st.data(), c->stream);
    if (rc != DISCO_OK) {
        c->err = own;
        return rc;
    }
    if (xrc != DISCO_OK) return fail(c, xrc, "%s: status exchange: %s", who, c->comm->err.c_str());
    for (size_t p = 0; p < G; p++)
        if ((int64_t)st[p] != DISCO_OK) return fail(c, (int)(int64_t)st[p], "%s: rank %zu could not do its part (code %d): no rank keeps its text", who, p, (int)(int64_t)st[p]);
    return DISCO_OK;
}

/* the contained-read lines: a rank's files are one range of containing reads, whose contained reads arrived anywhere. The reduced keys
 * — every rank holds those of its home slice — are brought together by ONE all-gather (per x 8 bytes per rank, the volume of the pass's
 * own reduce-scatter), in place: the other slices of best[] hold nothing anybody reads after the pass, and the next pass fills the table
 * afresh. Everything behind the gather is the rank's own business; the ranks compare notes at the end */
int64_t disco_dist_format_contained(disco_ctx *c, uint32_t n_files, const uint64_t *file_index, uint64_t *file_offsets)
{
    DISCO_TRACE("disco_dist_format_contained");
    if (!c || !file_offsets || n_files == 0) return DISCO_E_ARG;
    if (!c->comm) return fail(c, DISCO_E_STATE, "disco_dist_format_contained: no communicator (one GPU: disco_format_contained)");
    if (!c->dist_reads || c->phase < 8) return fail(c, DISCO_E_STATE, "disco_dist_format_contained: run disco_dist_run_graph first");
    if (c->n >= (1ull << 31)) return fail(c, DISCO_E_UNSUPPORTED, "disco_dist_format_contained: more than 2^31 reads");
    HIPCHK(c, hipSetDevice(c->device));
    for (uint32_t f = 0; f <= n_files; f++) file_offsets[f] = 0;
    c->ctext.bytes = 0;
    c->ctext.off.assign((size_t)n_files + 1, 0);
    const u64 G = (u64)c->comm->world, r = (u64)c->comm->rank, n = c->n, F = n_files;
    if (c->d_best.cap < c->per * G) return fail(c, DISCO_E_STATE, "disco_dist_format_contained: the containment keys of the last pass are gone");
    CHK(settle_keys(c));
    COMM_CHK(c, c->comm->all_gather(c->d_best + r * c->per, c->d_best, c->per * 8, c->stream));
    uint32_t f_lo, f_hi;
    dist_own_files(c, n_files, &f_lo, &f_hi);
    const u64 s_lo = ((u64)f_lo * n + F - 1) / F, s_hi = ((u64)f_hi * n + F - 1) / F; /* file t begins at the read ceil(t n / F) */
    if (getenv("DISCO_VERBOSE"))
        fprintf(stderr, "[disco] rank %llu of %llu: contained-read files [%u, %u) of %u, containing reads [%llu, %llu); keys gathered, %llu bytes to the other ranks\n",
                (unsigned long long)r, (unsigned long long)G, f_lo, f_hi, n_files, (unsigned long long)s_lo, (unsigned long long)s_hi, (unsigned long long)((G - 1) * c->per * 8));
    const int64_t nb = s_hi <= s_lo ? 0 : format_contained_rows(c, "disco_dist_format_contained", n_files, file_index, file_offsets, nullptr, s_lo, s_hi, 0);
    const int rc = dist_agree(c, "disco_dist_format_contained", nb < 0 ? (int)nb : DISCO_OK);
    if (rc != DISCO_OK) {
        for (uint32_t f = 0; f <= n_files; f++) file_offsets[f] = 0;
        c->ctext.bytes = 0;
        c->ctext.off.assign((size_t)n_files + 1, 0);
        return rc;
    }
    return nb;
}

/* the buffers of disco_dist_format_edges and the figures its steps share */
struct DistEdgeText {
    LocalBuf<u32> src32;
    LocalBuf<u64> src, ent, d_findex, within, place;
    LocalBuf<u8> bytes, sel;
    LocalBuf<u16> efile;
    uint32_t n_files = 0, f_lo = 0, f_hi = 0; /* the rank's files: [f_lo, f_hi) */
    u64 ne = 0;                              /* edges of the job */
    explicit DistEdgeText(disco_ctx *c) : src32(c), src(c), ent(c), d_findex(c), within(c), place(c), bytes(c), sel(c), efile(c) {}
};

/* 2. everything the rank will need, and its own edges compacted to where they lie in the job's list (from first_own on) */
static int dist_edge_text_prepare(disco_ctx *c, DistEdgeText &T, const uint64_t *file_index, u64 first_own)
{
    const u64 ne = T.ne, ne_own = c->n_out;
    CHK(ensure(c, T.src32, ne));
    CHK(ensure(c, T.ent, ne));
    CHK(ensure(c, T.src, ne));
    CHK(ensure(c, T.efile, ne));
    CHK(ensure(c, T.bytes, ne));
    if (T.f_hi > T.f_lo) {
        CHK(ensure(c, T.sel, ne));
        CHK(ensure(c, T.within, ne + 1));
        CHK(ensure(c, T.place, ne));
    }
    if (file_index) {
        CHK(ensure(c, T.d_findex, c->n));
        HIPCHK(c, hipMemcpyAsync(T.d_findex, file_index, c->n * 8, hipMemcpyHostToDevice, c->stream));
    }
    if (ne_own) {
        if (c->out_dense) {
            hipLaunchKernelGGL(emit_src32_kernel, dim3(flat_grid(c, ne_own)), dim3(256), 0, c->stream, c->d_out_src, ne_own, T.src32.p + first_own);
            HIPCHK(c, hipMemcpyAsync(T.ent.p + first_own, c->d_out_ent, ne_own * 8, hipMemcpyDeviceToDevice, c->stream));
        } else
            hipLaunchKernelGGL(emit_compact32_kernel, dim3(flat_grid(c, c->out_used)), dim3(256), 0, c->stream, c->d_out_src, c->d_out_ent, c->d_out_valid, c->d_out_pos, c->out_used,
                               T.src32.p + first_own, T.ent.p + first_own);
        HIPCHK(c, hipGetLastError());
    }
    return DISCO_OK;
}

/* steps 2 to 5 of disco_dist_format_edges. *gathered: every rank is past the first verdict, so all of them meet again at the end */
static int dist_edge_text(disco_ctx *c, DistEdgeText &T, const uint64_t *file_index, const std::vector<u64> &cnt, const std::vector<u64> &first, bool *gathered)
{
    const size_t G = (size_t)c->comm->world, r = (size_t)c->comm->rank;
    const u64 ne = T.ne;
    CHK(dist_agree(c, "disco_dist_format_edges", dist_edge_text_prepare(c, T, file_index, first[r])));
    *gathered = true;
    /* 3. the job's edges on every rank, in the order of the ranks */
    std::vector<size_t> off(G), len(G);
    for (size_t p = 0; p < G; p++) {
        off[p] = (size_t)first[p] * 4;
        len[p] = (size_t)cnt[p] * 4;
    }
    COMM_CHK(c, c->comm->all_gather_v(T.src32.p + first[r], T.src32.p, off.data(), len.data(), c->stream));
    for (size_t p = 0; p < G; p++) {
        off[p] *= 2;
        len[p] *= 2;
    }
    COMM_CHK(c, c->comm->all_gather_v(T.ent.p + first[r], T.ent.p, off.data(), len.data(), c->stream));
    hipLaunchKernelGGL(text_widen_src_kernel, dim3(flat_grid(c, ne)), dim3(256), 0, c->stream, (const u32 *)T.src32, ne, T.src.p);
    HIPCHK(c, hipGetLastError());
    /* 4. the files of the edges: on the device they stay */
    const int64_t part = partition_edges(c, T.src, T.ent, nullptr, nullptr, ne, ne, c->n, T.n_files, nullptr, T.efile.p);
    if (part < 0) return (int)part;
    /* 5. all lines measured; those of the rank's files placed and written */
    TextView g;
    g.src = T.src;
    g.ent = T.ent;
    g.valid = nullptr;
    g.pos = nullptr;
    g.len = c->d_len;
    g.file_index = T.d_findex;
    g.n_slots = ne;
    CHK(place_edge_lines(c, g, ne, T.efile, T.n_files, T.f_lo, T.f_hi, T.bytes, T.sel, T.within, T.place, (uint64_t *)c->text.off.data()));
    const u64 base = c->text.off[T.n_files];
    CHK(ensure(c, c->text.d, std::max<u64>(base, 1)));
    if (base)
        hipLaunchKernelGGL(text_write_owned_kernel, dim3(flat_grid(c, ne)), dim3(256), 0, c->stream, g, (const u64 *)T.place, (const u16 *)T.efile, T.f_lo, T.f_hi, c->text.d.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->text.bytes = base;
    return DISCO_OK;
}

/* the edge lines: the ranks' edges — compacted, 12 bytes each — are all-gathered, every rank cuts the same files out of the same list
 * (partition_edges: the assignment depends on the set of edges alone), measures every line and places and writes those of its own files.
 * What the gather needs — the rank's memory — is there before the rank enters it, and the ranks exchange a status word in front of it:
 * either all of them gather, or none; and again at the end, for what every rank did alone behind it */
int64_t disco_dist_format_edges(disco_ctx *c, uint32_t n_files, const uint64_t *file_index, uint64_t *file_offsets)
{
    DISCO_TRACE("disco_dist_format_edges");
    if (!c || !file_offsets || n_files == 0) return DISCO_E_ARG;
    if (!c->comm) return fail(c, DISCO_E_STATE, "disco_dist_format_edges: no communicator (one GPU: disco_format_edges)");
    if (!c->dist_reads || c->phase < 8) return fail(c, DISCO_E_STATE, "disco_dist_format_edges: run disco_dist_run_graph first");
    if (n_files > 256) return fail(c, DISCO_E_UNSUPPORTED, "disco_dist_format_edges: more than 256 files (one placement pass per file)");
    if (c->prm.max_substitutions) return fail(c, DISCO_E_UNSUPPORTED, "disco_dist_format_edges: the substitutions column is written by the host writer");
    if (c->n >= (1ull << 31)) return fail(c, DISCO_E_UNSUPPORTED, "disco_dist_format_edges: more than 2^31 reads");
    HIPCHK(c, hipSetDevice(c->device));
    for (uint32_t f = 0; f <= n_files; f++) file_offsets[f] = 0;
    c->text.bytes = 0;
    c->text.off.assign((size_t)n_files + 1, 0);
    const size_t G = (size_t)c->comm->world, r = (size_t)c->comm->rank;
    const u64 ne_own = c->n_out;
    /* 1. who has how many edges */
    std::vector<u64> cnt(G);
    {
        const u64 mine = ne_own;
        COMM_CHK(c, c->comm->host_all_gather((const unsigned long long *)&mine, 1, (unsigned long long *)cnt.data(), c->stream));
    }
    std::vector<u64> first(G + 1, 0);
    for (size_t p = 0; p < G; p++) first[p + 1] = first[p] + cnt[p];
    const u64 ne = first[G];
    if (ne == 0) return 0;
    uint32_t f_lo, f_hi;
    dist_own_files(c, n_files, &f_lo, &f_hi);
    DistEdgeText T(c);
    T.n_files = n_files;
    T.f_lo = f_lo;
    T.f_hi = f_hi;
    T.ne = ne;
    bool gathered = false;
    int rc = dist_edge_text(c, T, file_index, cnt, first, &gathered);
    if (gathered) rc = dist_agree(c, "disco_dist_format_edges", rc);
    if (rc != DISCO_OK) {
        c->text.bytes = 0;
        c->text.off.assign((size_t)n_files + 1, 0);
        return rc;
    }
    for (uint32_t f = 0; f <= n_files; f++) file_offsets[f] = c->text.off[f];
    if (getenv("DISCO_VERBOSE"))
        fprintf(stderr, "[disco] rank %zu of %zu: edge files [%u, %u) of %u, %llu bytes of %llu edges' lines; edges gathered, %llu bytes to the other ranks\n", r, G, f_lo, f_hi, n_files,
                (unsigned long long)c->text.bytes, (unsigned long long)ne, (unsigned long long)((G - 1) * ne_own * 12));
    return (int64_t)c->text.bytes;
}

} /* extern "C" */
