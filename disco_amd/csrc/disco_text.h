/*
 * disco_text.h — the edge lines of the stage's text files formatted on the GPU (saveParGraphToFile, BG/OverlapGraph.cpp:808-867):
 *     src \t dst \t orient,ovl,0,0,len1,start1,len1-1,len2,0,ovl-1,NA,2 \n          src < dst, 1-based file indices
 * 45 M edges are 2.5 GB of decimal numbers: 16 host threads need a second for them, the GPU a few milliseconds — one thread per
 * edge measures its line, a scan per file places it, the same thread writes it. The files come out byte for byte as
 * disco_amd/host/writer.cpp writes them (edges of a file in fetch order, every line with flag 2: the files are cut along connected
 * components), which is what tests/test_host.py compares.
 */
#ifndef DISCO_TEXT_H_
#define DISCO_TEXT_H_

#include "disco_kernels.h"

struct TextView {
    const u64 *src, *ent;
    const u8 *valid;
    const u64 *pos;
    const u16 *len;
    const u64 *file_index; /* [n] or null: id + 1 */
    u64 n_slots;
};

__device__ __forceinline__ u32 tx_digits(u64 v)
{
    u32 d = 1;
    while (v >= 10) {
        v /= 10;
        d++;
    }
    return d;
}
__device__ __forceinline__ char *tx_put(char *p, u64 v)
{
    const u32 d = tx_digits(v);
    for (u32 i = d; i-- > 0;) {
        p[i] = (char)('0' + (u32)(v % 10));
        v /= 10;
    }
    return p + d;
}
struct TextNumbers {
    u64 a, b;
    u32 orient, ovl, len1, off, len2;
};
__device__ __forceinline__ TextNumbers tx_numbers(const TextView &g, u64 s)
{
    TextNumbers t;
    const u64 src = g.src[s], e = g.ent[s], dst = ADJ_DST(e);
    t.a = g.file_index ? g.file_index[src] : src + 1;
    t.b = g.file_index ? g.file_index[dst] : dst + 1;
    t.orient = ADJ_ORI(e);
    t.len1 = g.len[src];
    t.off = ADJ_OFF(e);
    t.ovl = t.len1 - t.off; /* :814 */
    t.len2 = ADJ_DLEN(e);
    return t;
}

/* bytes of every edge's line, by the edge's rank in fetch order */
__global__ void text_measure_kernel(TextView g, u8 *__restrict__ bytes)
{
    u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; s < g.n_slots; s += (u64)gridDim.x * blockDim.x) {
        if (g.valid && !g.valid[s]) continue;
        const TextNumbers t = tx_numbers(g, s);
        /* a \t b \t o , ovl ,0,0, len1 , off , len1-1 , len2 ,0, ovl-1 ,NA,2 \n  : 20 fixed characters + the orientation digit */
        bytes[g.pos ? g.pos[s] : s] = (u8)(tx_digits(t.a) + tx_digits(t.b) + 1 + tx_digits(t.ovl) + tx_digits(t.len1) + tx_digits(t.off) + tx_digits(t.len1 - 1) + tx_digits(t.len2) +
                               tx_digits(t.ovl - 1) + 20);
    }
}

/* the lines of one file: their lengths, 0 for the edges of other files (scanned into offsets inside the file) */
__global__ void text_select_kernel(const u8 *__restrict__ bytes, const u16 *__restrict__ efile, u64 ne, u32 file, u8 *__restrict__ out)
{
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i < ne; i += (u64)gridDim.x * blockDim.x) out[i] = efile[i] == file ? bytes[i] : (u8)0;
}
__global__ void text_place_kernel(const u64 *__restrict__ within, const u16 *__restrict__ efile, u64 ne, u32 file, u64 base, u64 *__restrict__ place)
{
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i < ne; i += (u64)gridDim.x * blockDim.x)
        if (efile[i] == file) place[i] = base + within[i];
}

/* one edge line at p */
__device__ __forceinline__ void tx_put_line(char *p, const TextNumbers &t)
{
    p = tx_put(p, t.a); *p++ = '\t';
    p = tx_put(p, t.b); *p++ = '\t';
    *p++ = (char)('0' + t.orient); *p++ = ',';
    p = tx_put(p, t.ovl); *p++ = ','; *p++ = '0'; *p++ = ','; *p++ = '0'; *p++ = ','; /* :815-816 substitutions, edits */
    p = tx_put(p, t.len1); *p++ = ',';
    p = tx_put(p, t.off); *p++ = ',';
    p = tx_put(p, t.len1 - 1); *p++ = ',';
    p = tx_put(p, t.len2); *p++ = ','; *p++ = '0'; *p++ = ',';
    p = tx_put(p, t.ovl - 1); *p++ = ','; *p++ = 'N'; *p++ = 'A'; *p++ = ','; *p++ = '2'; *p++ = '\n';
}

__global__ void text_write_kernel(TextView g, const u64 *__restrict__ place, char *__restrict__ text)
{
    u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; s < g.n_slots; s += (u64)gridDim.x * blockDim.x) {
        if (g.valid && !g.valid[s]) continue;
        const TextNumbers t = tx_numbers(g, s);
        tx_put_line(text + place[g.pos ? g.pos[s] : s], t);
    }
}

/* ---- a rank of a multi-GPU job writes the files [f_lo, f_hi) only (disco_dist_format_edges): the edges of all ranks lie on every rank,
 * gathered with their sources as 32 bits; every line is measured, the lines of the rank's files are placed and written ---- */
__global__ void text_widen_src_kernel(const u32 *__restrict__ src32, u64 ne, u64 *__restrict__ src)
{
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i < ne; i += (u64)gridDim.x * blockDim.x) src[i] = src32[i];
}
/* text_write_kernel behind a file-ownership mask: place[] of an edge of another rank's file was never set, and is never read */
__global__ void text_write_owned_kernel(TextView g, const u64 *__restrict__ place, const u16 *__restrict__ efile, u32 f_lo, u32 f_hi, char *__restrict__ text)
{
    u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; s < g.n_slots; s += (u64)gridDim.x * blockDim.x) {
        if (g.valid && !g.valid[s]) continue;
        const u64 e = g.pos ? g.pos[s] : s;
        const u32 f = efile[e];
        if (f < f_lo || f >= f_hi) continue;
        const TextNumbers t = tx_numbers(g, s);
        tx_put_line(text + place[e], t);
    }
}

/* ================================================================================================================================
 * the lines of <prefix>_<t>_containedReads.txt (BG/OverlapGraph.cpp:438-447; disco_amd/host/writer.cpp write_contained):
 *     contained \t super \t orient,len2,0,0,len2,0,len2,len1,start,start+len2 \n                       1-based file indices
 * in ascending (containing read, j, contained read) — sort_contained's order, SG/DataSet.cpp:316-335 — file t holding the containing
 * reads s with floor(s * n_files / n) == t. Straight from best[] and the contained flags: a counting sort by containing read (count,
 * scan, place), then every group sorted by ONE 64-bit word per row — the containing read is the group's — whatever its size:
 *     up to CROW_GROUP_MAX rows        one thread per group, insertion sort (a handful of rows nearly always)
 *     up to CGRP_LDS_MAX rows          listed; one workgroup per listed group, bitonic network in LDS
 *     beyond                           listed; one workgroup per listed group, the same network on the group where it lies: chunks of
 *                                      CGRP_LDS_MAX rows through LDS for every step that stays inside a chunk, global memory for the rest
 * then measure -> scan -> write as for the edges, one thread per grouped row. Sorted by containing read the rows of a file are
 * contiguous: its first byte is the place of the first row of its first containing read, no pass per file.
 * ============================================================================================================================== */
#define CWORD_MAKE(j, id, suf, rev) (((u64)(j) << 33) | ((u64)(id) << 2) | ((u64)(suf) << 1) | (u64)(rev)) /* j(15) | contained id(31) | suffix | rev */
#define CWORD_J(w) ((u32)((w) >> 33) & 0x7FFFu)
#define CWORD_ID(w) (((w) >> 2) & 0x7FFFFFFFull)
#define CGRP_LDS_MAX 4096u /* rows: 32 KiB of LDS per workgroup, so five workgroups share a CU's 160 KiB */
#define CGRP_BLOCK 256
enum { CGRP_N_LDS = 0, CGRP_N_GLOBAL = 1, CGRP_LARGEST = 2, CGRP_BAD_KEYS = 3, CGRP_CTRS = 4 };

/* (a key that names no read must not index anything: counted, and the caller fails loudly) */
__global__ void cgrp_count_kernel(const u64 *__restrict__ best, const u8 *__restrict__ contained, u64 n, u32 *__restrict__ cnt, u32 *__restrict__ ctr)
{
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i < n; i += (u64)gridDim.x * blockDim.x)
        if (contained[i]) {
            const u64 s = CKEY_SUPER(best[i]);
            if (s < n) atomicAdd(&cnt[s], 1u);
            else atomicAdd(&ctr[CGRP_BAD_KEYS], 1u);
        }
}
/* cursor = the exclusive scan of cnt (consumed: afterwards cursor[s] = end of group s, and its start is the end of group s - 1) */
__global__ void cgrp_place_kernel(const u64 *__restrict__ best, const u8 *__restrict__ contained, u64 n, u64 nc, u32 *__restrict__ cursor, u64 *__restrict__ word,
                                  u32 *__restrict__ sup)
{
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i < n; i += (u64)gridDim.x * blockDim.x)
        if (contained[i]) {
            const u64 key = best[i], s = CKEY_SUPER(key);
            if (s >= n) continue;
            const u32 at = atomicAdd(&cursor[s], 1u);
            if (at >= nc) continue; /* (flags and keys that do not agree with the count: never past the arrays) */
            word[at] = CWORD_MAKE(CKEY_J(key), i, CKEY_SUFFIX(key), CKEY_REV(key));
            sup[at] = (u32)s;
        }
}

/* the range-restricted forms (disco_dist_format_contained): a rank of a multi-GPU job groups the rows whose containing read lies in
 * [s_lo, s_hi) — the reads of the files it writes — out of the keys of ALL reads, all-gathered. Who is contained is read off the key
 * (the flags of a rank cover its home range only); cnt / cursor stay indexed by read id, zero outside the range, so that everything
 * behind them (the sorts, ctext_offsets_kernel) runs unchanged and a file of another rank comes out empty */
__global__ void cgrp_count_range_kernel(const u64 *__restrict__ best, u64 n, u64 s_lo, u64 s_hi, u32 *__restrict__ cnt, u32 *__restrict__ ctr)
{
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u64 key = best[i];
        if (key == DISCO_NOKEY) continue;
        const u64 s = CKEY_SUPER(key);
        if (s >= n) atomicAdd(&ctr[CGRP_BAD_KEYS], 1u);
        else if (s >= s_lo && s < s_hi) atomicAdd(&cnt[s], 1u);
    }
}
__global__ void cgrp_place_range_kernel(const u64 *__restrict__ best, u64 n, u64 s_lo, u64 s_hi, u64 nc, u32 *__restrict__ cursor, u64 *__restrict__ word, u32 *__restrict__ sup)
{
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u64 key = best[i];
        if (key == DISCO_NOKEY) continue;
        const u64 s = CKEY_SUPER(key);
        if (s < s_lo || s >= s_hi) continue; /* (s_hi <= n) */
        const u32 at = atomicAdd(&cursor[s], 1u);
        if (at >= nc) continue;
        word[at] = CWORD_MAKE(CKEY_J(key), i, CKEY_SUFFIX(key), CKEY_REV(key));
        sup[at] = (u32)s;
    }
}

struct CgrpLists {
    u32 *lds, *glb; /* containing reads of the groups beyond CROW_GROUP_MAX / beyond CGRP_LDS_MAX rows */
    u32 *ctr;       /* [CGRP_CTRS] */
    u32 cap;        /* entries of either list */
};
/* one thread per containing read: small groups sorted here, the others listed for the kernels below */
__global__ void cgrp_sort_small_kernel(const u32 *__restrict__ gend, u64 n, u64 *__restrict__ word, CgrpLists L)
{
    u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u32 largest = 0;
    for (; s < n; s += (u64)gridDim.x * blockDim.x) {
        const u32 b = s ? gend[s - 1] : 0u, e = gend[s], m = e - b;
        largest = m > largest ? m : largest;
        if (m < 2) continue;
        if (m > CROW_GROUP_MAX) {
            const bool in_lds = m <= CGRP_LDS_MAX;
            const u32 at = atomicAdd(&L.ctr[in_lds ? CGRP_N_LDS : CGRP_N_GLOBAL], 1u);
            if (at < L.cap) (in_lds ? L.lds : L.glb)[at] = (u32)s;
            continue;
        }
        for (u32 a = b + 1; a < e; a++) {
            const u64 w = word[a];
            u32 q = a;
            while (q > b && word[q - 1] > w) {
                word[q] = word[q - 1];
                q--;
            }
            word[q] = w;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const u32 x = __shfl_down(largest, o);
        largest = x > largest ? x : largest;
    }
    if ((threadIdx.x & 63) == 0 && largest > __atomic_load_n(&L.ctr[CGRP_LARGEST], __ATOMIC_RELAXED)) atomicMax(&L.ctr[CGRP_LARGEST], largest); /* (a figure for the log) */
}

/* One step of a bitonic network on h[0..m) whose compare-exchanges ALL put the smaller word at the smaller index: merge k2 begins with
 * its mirror step (j2 == 0: i against i ^ (k2 - 1)) and goes on with the half-distances j2 = k2 / 4 ... 1 (i against i + j2). Rows at
 * m and beyond count as +infinity: they would never move, so their exchanges are skipped and m needs no padding to the power of two P. */
__host__ __device__ __forceinline__ void cgrp_step(u64 *h, u32 m, u32 P, u32 k2, u32 j2, u32 tid, u32 nt)
{
    for (u32 t = tid; t < P / 2; t += nt) {
        u32 i, p;
        if (j2 == 0) {
            const u32 r = t & ((k2 >> 1) - 1);
            i = 2 * (t - r) + r;
            p = i + (k2 - 1 - 2 * r);
        } else {
            i = 2 * t - (t & (j2 - 1));
            p = i + j2;
        }
        if (p < m) {
            const u64 x = h[i], y = h[p];
            if (x > y) {
                h[i] = y;
                h[p] = x;
            }
        }
    }
}
__host__ __device__ __forceinline__ u32 cgrp_pow2(u32 m)
{
    u32 P = 2;
    while (P < m) P <<= 1;
    return P;
}
#if defined(__HIP_DEVICE_COMPILE__)
#define CGRP_SYNC() __syncthreads()
#else
#define CGRP_SYNC() ((void)0)
#endif
/* all merges up to k_hi of h[0..m), by the nt threads of a workgroup */
__host__ __device__ __forceinline__ void cgrp_sort_lds(u64 *h, u32 m, u32 k_hi, u32 tid, u32 nt)
{
    for (u32 k2 = 2; k2 <= k_hi; k2 <<= 1) {
        cgrp_step(h, m, k_hi, k2, 0, tid, nt);
        CGRP_SYNC();
        for (u32 j2 = k2 >> 2; j2 > 0; j2 >>= 1) {
            cgrp_step(h, m, k_hi, k2, j2, tid, nt);
            CGRP_SYNC();
        }
    }
}

/* one workgroup per listed group of up to CGRP_LDS_MAX rows */
__global__ __launch_bounds__(CGRP_BLOCK) void cgrp_sort_lds_kernel(const u32 *__restrict__ gend, u64 *__restrict__ word, CgrpLists L)
{
    __shared__ u64 h[CGRP_LDS_MAX];
    const u32 n_list = min(L.ctr[CGRP_N_LDS], L.cap);
    for (u32 g = blockIdx.x; g < n_list; g += gridDim.x) {
        const u32 s = L.lds[g], b = s ? gend[s - 1] : 0u, m = min(gend[s] - b, CGRP_LDS_MAX);
        for (u32 i = threadIdx.x; i < m; i += CGRP_BLOCK) h[i] = word[b + i];
        __syncthreads();
        cgrp_sort_lds(h, m, cgrp_pow2(m), threadIdx.x, CGRP_BLOCK);
        for (u32 i = threadIdx.x; i < m; i += CGRP_BLOCK) word[b + i] = h[i];
        __syncthreads();
    }
}

/* one workgroup per listed group beyond that: the network's steps at distances below CGRP_LDS_MAX stay inside aligned chunks of
 * CGRP_LDS_MAX rows and run in LDS, chunk after chunk; the mirror steps and half-distances from CGRP_LDS_MAX up run on the group in
 * global memory (the workgroup's barrier orders them: one CU, one L1). A group of 2^16 rows: 10 steps through global memory, 5 sweeps
 * through LDS */
__global__ __launch_bounds__(CGRP_BLOCK) void cgrp_sort_global_kernel(const u32 *__restrict__ gend, u64 *word, CgrpLists L)
{
    __shared__ u64 h[CGRP_LDS_MAX];
    const u32 n_list = min(L.ctr[CGRP_N_GLOBAL], L.cap), tid = threadIdx.x;
    for (u32 g = blockIdx.x; g < n_list; g += gridDim.x) {
        const u32 s = L.glb[g], b = s ? gend[s - 1] : 0u, m = gend[s] - b;
        u64 *w = word + b;
        const u64 P = cgrp_pow2(m); /* (m < 2^31: P fits 32 bits, the loop variable that passes it does not) */
        for (u64 k2 = CGRP_LDS_MAX; k2 <= P; k2 <<= 1) {
            if (k2 > CGRP_LDS_MAX) {
                cgrp_step(w, m, (u32)P, (u32)k2, 0, tid, CGRP_BLOCK);
                __syncthreads();
                for (u32 j2 = (u32)(k2 >> 2); j2 >= CGRP_LDS_MAX; j2 >>= 1) {
                    cgrp_step(w, m, (u32)P, (u32)k2, j2, tid, CGRP_BLOCK);
                    __syncthreads();
                }
            }
            for (u32 c0 = 0; c0 < m; c0 += CGRP_LDS_MAX) {
                const u32 mm = min(m - c0, CGRP_LDS_MAX);
                for (u32 i = tid; i < mm; i += CGRP_BLOCK) h[i] = w[c0 + i];
                __syncthreads();
                if (k2 == CGRP_LDS_MAX) cgrp_sort_lds(h, mm, CGRP_LDS_MAX, tid, CGRP_BLOCK); /* every chunk sorted: the merges up to CGRP_LDS_MAX */
                else
                    for (u32 j2 = CGRP_LDS_MAX >> 1; j2 > 0; j2 >>= 1) {
                        cgrp_step(h, mm, CGRP_LDS_MAX, (u32)k2, j2, tid, CGRP_BLOCK);
                        __syncthreads();
                    }
                for (u32 i = tid; i < mm; i += CGRP_BLOCK) w[c0 + i] = h[i];
                __syncthreads();
            }
        }
    }
}

struct CTextView {
    const u64 *word; /* grouped rows */
    const u32 *sup;  /* their containing reads */
    const u16 *len;
    const u64 *file_index; /* [n] or null: id + 1 */
    u64 nc;
    u32 k;
};
struct CTextNumbers {
    u64 a, b;
    u32 orient, len1, len2, start;
};
__device__ __forceinline__ CTextNumbers ctx_numbers(const CTextView &g, u64 i)
{
    CTextNumbers t;
    const u64 w = g.word[i], id = CWORD_ID(w), s = g.sup[i];
    t.a = g.file_index ? g.file_index[id] : id + 1;
    t.b = g.file_index ? g.file_index[s] : s + 1;
    t.len2 = g.len[id];
    t.len1 = g.len[s];
    disco_map_type(disco_hit_type((u32)(w >> 1) & 1u, (u32)w & 1u), t.len1, g.k, CWORD_J(w), &t.orient, &t.start); /* BG/OverlapGraph.cpp:428-434 */
    return t;
}
__global__ void ctext_measure_kernel(CTextView g, u8 *__restrict__ bytes)
{
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i < g.nc; i += (u64)gridDim.x * blockDim.x) {
        const CTextNumbers t = ctx_numbers(g, i);
        /* a \t b \t o , len2 ,0,0, len2 ,0, len2 , len1 , start , start+len2 \n  : 15 fixed characters + the orientation digit */
        bytes[i] = (u8)(tx_digits(t.a) + tx_digits(t.b) + 1 + 3 * tx_digits(t.len2) + tx_digits(t.len1) + tx_digits(t.start) + tx_digits(t.start + t.len2) + 15);
    }
}
/* first byte of every file (and, for file n_files, the end of the text): place[] of the first row of the first containing read the
 * file owns — the reads from ceil(t n / n_files) on; place has nc + 1 entries, the last one the total */
__global__ void ctext_offsets_kernel(const u32 *__restrict__ gend, u64 n, u64 nc, const u64 *__restrict__ place, u32 n_files, u64 *__restrict__ off)
{
    u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; t <= n_files; t += (u64)gridDim.x * blockDim.x) {
        const u64 first = (t * n + n_files - 1) / n_files;
        const u64 row = first == 0 ? 0 : (first >= n ? nc : (u64)gend[first - 1]);
        off[t] = place[row < nc ? row : nc];
    }
}
__global__ void ctext_write_kernel(CTextView g, const u64 *__restrict__ place, char *__restrict__ text)
{
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i < g.nc; i += (u64)gridDim.x * blockDim.x) {
        const CTextNumbers t = ctx_numbers(g, i);
        char *p = text + place[i];
        p = tx_put(p, t.a); *p++ = '\t';
        p = tx_put(p, t.b); *p++ = '\t';
        *p++ = (char)('0' + t.orient); *p++ = ',';
        p = tx_put(p, t.len2); *p++ = ','; *p++ = '0'; *p++ = ','; *p++ = '0'; *p++ = ',';
        p = tx_put(p, t.len2); *p++ = ','; *p++ = '0'; *p++ = ',';
        p = tx_put(p, t.len2); *p++ = ',';
        p = tx_put(p, t.len1); *p++ = ',';
        p = tx_put(p, t.start); *p++ = ',';
        p = tx_put(p, t.start + t.len2); *p++ = '\n';
    }
}

#endif /* DISCO_TEXT_H_ */
