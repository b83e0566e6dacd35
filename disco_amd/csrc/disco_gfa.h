/*
 * disco_gfa.h — the overlap graph as GFA 1.0, formatted on the GPU (<prefix>.gfa; disco_write_gfa, include/disco_hip.h):
 *     H \t VN:Z:1.0
 *     S \t name \t bases \t LN:i:len                       one per read, in read-id order (bases = * without sequences)
 *     L \t src \t so \t dst \t do \t ovl M [\t NM:i:n]       one per reduced edge, in the order of disco_fetch_edges
 *     C \t container \t + \t contained \t o \t pos \t len2 M one per contained-read row, in the order of the contained-read files
 * names are 1-based file indices (the ids of every other file this stage writes). Orientations (BG/Edge.h:30-34,
 * BG/OverlapGraph.cpp:660-667): so = '+' when orient & 2, do = '+' when orient & 1, ovl = len(src) - offset — the suffix of oriented src of
 * ovl bases is the prefix of oriented dst. A contained row (BG/OverlapGraph.cpp:428-434) of orientation 0 or 3 lies forward in its
 * container, 1 or 2 reversed; it begins at `start` for 3 and 2 (the k-mer hit its oriented prefix) and at len1 - start - len2 for 0 and 1
 * (the hit was its oriented suffix, which ends at j + k = len1 - start).
 *
 * Measure -> scan -> write, as for the other three texts (disco_text.h, disco_partext.h), with two differences. The text is never
 * resident: it is cut at line ends into pieces that fit a half of the pinned ring, and a write kernel fills one piece (gfa_cuts_kernel
 * finds the cuts in the scanned line starts). And the S lines, which are nearly all of the bytes, are not written one lane per line: a
 * lane is one 32-base WORD of a read and writes its 32 characters, so the lanes of a wavefront that share a read store one contiguous
 * run. A line begins wherever the one before it ended, so a lane's 32 bytes start at any address: gfa_store cuts them into naturally
 * aligned stores, the widest the address allows — 1, 2, 4, 8 bytes up to the first 16-byte boundary, 16-byte stores from there, and
 * the same ladder down at the ragged end (at most 6 stores for 32 bytes, 2 where the line happens to be aligned). The lane of word 0
 * also writes "S \t name \t", the lane of the last word "\t LN:i:len \n". The table's three layouts are one function (gfa_word): rows
 * of one stride, narrow or wide, and two classes of rows, where the words of a read of more than 256 bases come from its full row.
 *
 * The line and item functions are plain functions (host and device): disco_amd/host/gfa_check.cpp runs them without a GPU.
 *
 * The S and L kernels take an optional skip flag per read / per edge: <prefix>.unitigs.gfa (disco_gfa_chains.h) writes the reads and
 * edges that the chain contraction left outside its composite edges with them; disco_write_gfa passes none.
 */
#ifndef DISCO_GFA_H_
#define DISCO_GFA_H_

#include <stdint.h>
#include <string.h>

#include "../../include/disco_hip.h"

#if defined(__HIPCC__)
#define GFA_HD __host__ __device__ __forceinline__
#else
#define GFA_HD inline
#endif

#define GFA_SHORT_MAX 256   /* DISCO_SHORT_MAX: bases a 64-byte row holds */
#define GFA_HEAD_WORDS 8    /* ... in that many words */
#define GFA_MAX_LINE 32832u /* no line is longer: S \t 20 digits \t 32767 bases \t LN:i: 5 digits \n = 32803 bytes */
#define GFA_HEADER "H\tVN:Z:1.0\n"

struct GfaReads {
    const uint64_t *rows;     /* [n][S], 2-bit bases MSB first; with two classes the 64-byte rows (a long read's row holds its head) */
    const uint64_t *full;     /* two classes: [n_long][SL], the long reads' whole rows; null: one stride                            */
    const uint32_t *ovf;      /* two classes: long reads before read i                                                             */
    const uint32_t *long_ids; /* two classes: the read that is long read j                                                         */
    const uint16_t *len;
    const uint64_t *file_index; /* [n] or null: id + 1 */
    uint64_t n;
    uint32_t S, SL;
};

GFA_HD uint32_t gfa_digits(uint64_t v)
{
    uint32_t d = 1;
    while (v >= 10) {
        v /= 10;
        d++;
    }
    return d;
}
GFA_HD char *gfa_put(char *p, uint64_t v)
{
    const uint32_t d = gfa_digits(v);
    for (uint32_t i = d; i-- > 0;) {
        p[i] = (char)('0' + (uint32_t)(v % 10));
        v /= 10;
    }
    return p + d;
}
GFA_HD uint64_t gfa_name(const GfaReads &g, uint64_t i) { return g.file_index ? g.file_index[i] : i + 1; }
/* word w of read i, whichever layout holds it */
GFA_HD uint64_t gfa_word(const GfaReads &g, uint64_t i, uint32_t w)
{
    if (g.full && g.len[i] > GFA_SHORT_MAX) return g.full[(uint64_t)g.ovf[i] * g.SL + w];
    return g.rows[i * g.S + w];
}

/* ---- 32 bases as 32 characters ------------------------------------------------------------------------------------------------- */
struct GfaChunk {
    uint64_t q[4]; /* character i is byte i & 7 of q[i >> 3] (little endian: the order of the bytes in memory) */
};
GFA_HD GfaChunk gfa_decode32(uint64_t word)
{
    GfaChunk c;
    for (int k = 0; k < 4; k++) {
        uint64_t v = 0;
        for (int b = 0; b < 8; b++) {
            const uint32_t code = (uint32_t)(word >> (62 - 2 * (8 * k + b))) & 3u;
            v |= (uint64_t)((0x54474341u >> (8 * code)) & 0xFFu) << (8 * b); /* A C G T */
        }
        c.q[k] = v;
    }
    return c;
}
/* the characters [p, p + 8) of a chunk (beyond 32: zeros); selects, not an indexed array, so that the chunk stays in registers */
GFA_HD uint64_t gfa_take8(const GfaChunk &c, uint32_t p)
{
    const uint32_t k = p >> 3, sh = (p & 7u) * 8u;
    const uint64_t lo = k == 0 ? c.q[0] : k == 1 ? c.q[1] : k == 2 ? c.q[2] : k == 3 ? c.q[3] : 0ull;
    const uint64_t hi = k == 0 ? c.q[1] : k == 1 ? c.q[2] : k == 2 ? c.q[3] : 0ull;
    return sh ? (lo >> sh) | (hi << (64u - sh)) : lo;
}
/* the first nb characters of a chunk to dst, in naturally aligned stores: the widest that the address and what is left allow */
GFA_HD void gfa_store(char *dst, const GfaChunk &c, uint32_t nb)
{
    uint32_t p = 0;
    while (p < nb) {
        char *a = dst + p;
        const uint32_t al = (uint32_t)(uintptr_t)a, left = nb - p;
        const uint64_t v = gfa_take8(c, p);
        uint32_t sz;
        if (!(al & 15u) && left >= 16) sz = 16;
        else if (!(al & 7u) && left >= 8) sz = 8;
        else if (!(al & 3u) && left >= 4) sz = 4;
        else if (!(al & 1u) && left >= 2) sz = 2;
        else sz = 1;
#if defined(__HIP_DEVICE_COMPILE__)
        if (sz == 16) {
            const uint64_t v2 = gfa_take8(c, p + 8);
            *(uint4 *)a = make_uint4((uint32_t)v, (uint32_t)(v >> 32), (uint32_t)v2, (uint32_t)(v2 >> 32));
        } else if (sz == 8) *(uint64_t *)a = v;
        else if (sz == 4) *(uint32_t *)a = (uint32_t)v;
        else if (sz == 2) *(uint16_t *)a = (uint16_t)v;
        else *a = (char)v;
#else
        memcpy(a, &v, sz < 8 ? sz : 8);
        if (sz == 16) {
            const uint64_t v2 = gfa_take8(c, p + 8);
            memcpy(a + 8, &v2, 8);
        }
#endif
        p += sz;
    }
}

/* ---- S lines: an item is one word of a read (without sequences: the whole line) ------------------------------------------------ */
GFA_HD uint32_t gfa_s_items(uint32_t len, bool no_seq) { return no_seq ? 1u : (len + 31u) >> 5; }
GFA_HD uint32_t gfa_s_bytes(uint64_t name, uint32_t len, bool no_seq)
{
    /* S \t name \t bases \t LN:i: len \n : 10 fixed characters */
    return gfa_digits(name) + (no_seq ? 1u : len) + gfa_digits(len) + 10u;
}
/* item w of the line that begins at `line`; word = the read's word w (not looked at without sequences) */
GFA_HD void gfa_s_put(char *line, uint64_t name, uint32_t len, uint32_t w, uint64_t word, bool no_seq)
{
    const uint32_t pre = gfa_digits(name) + 3u, body = no_seq ? 1u : len;
    if (w == 0) {
        line[0] = 'S';
        line[1] = '\t';
        *gfa_put(line + 2, name) = '\t';
    }
    if (no_seq) line[pre] = '*';
    else {
        const uint32_t left = len - 32u * w;
        gfa_store(line + pre + 32u * w, gfa_decode32(word), left < 32u ? left : 32u);
    }
    if (w + 1 == gfa_s_items(len, no_seq)) {
        char *p = line + pre + body;
        *p++ = '\t'; *p++ = 'L'; *p++ = 'N'; *p++ = ':'; *p++ = 'i'; *p++ = ':';
        p = gfa_put(p, len);
        *p = '\n';
    }
}

/* ---- L lines ------------------------------------------------------------------------------------------------------------------- */
struct GfaL {
    uint64_t a, b; /* names of source and destination */
    uint32_t orient, ovl, nm;
    bool has_nm;
};
GFA_HD uint32_t gfa_l_bytes(const GfaL &t)
{
    /* L \t a \t so \t b \t do \t ovl M \n : 10 fixed characters; \t NM:i: n : 6 */
    return gfa_digits(t.a) + gfa_digits(t.b) + gfa_digits(t.ovl) + 10u + (t.has_nm ? 6u + gfa_digits(t.nm) : 0u);
}
GFA_HD char *gfa_l_put(char *p, const GfaL &t)
{
    *p++ = 'L'; *p++ = '\t';
    p = gfa_put(p, t.a); *p++ = '\t';
    *p++ = (t.orient & 2u) ? '+' : '-'; *p++ = '\t';
    p = gfa_put(p, t.b); *p++ = '\t';
    *p++ = (t.orient & 1u) ? '+' : '-'; *p++ = '\t';
    p = gfa_put(p, t.ovl); *p++ = 'M';
    if (t.has_nm) {
        *p++ = '\t'; *p++ = 'N'; *p++ = 'M'; *p++ = ':'; *p++ = 'i'; *p++ = ':';
        p = gfa_put(p, t.nm);
    }
    *p++ = '\n';
    return p;
}

/* ---- C lines ------------------------------------------------------------------------------------------------------------------- */
struct GfaC {
    uint64_t a, b; /* names of the containing and of the contained read */
    uint32_t minus, pos, len2;
};
/* from a contained row's numbers (disco_contained_row: orient, len1, len2, start = len1 - overlapLen) */
GFA_HD GfaC gfa_c_of(uint64_t container, uint64_t contained, uint32_t orient, uint32_t len1, uint32_t len2, uint32_t start)
{
    GfaC t;
    t.a = container;
    t.b = contained;
    t.minus = (orient == 1u || orient == 2u) ? 1u : 0u;
    t.pos = (orient & 2u) ? start : len1 - start - len2;
    t.len2 = len2;
    return t;
}
GFA_HD uint32_t gfa_c_bytes(const GfaC &t)
{
    /* C \t a \t + \t b \t o \t pos \t len2 M \n : 11 fixed characters */
    return gfa_digits(t.a) + gfa_digits(t.b) + gfa_digits(t.pos) + gfa_digits(t.len2) + 11u;
}
GFA_HD char *gfa_c_put(char *p, const GfaC &t)
{
    *p++ = 'C'; *p++ = '\t';
    p = gfa_put(p, t.a); *p++ = '\t'; *p++ = '+'; *p++ = '\t';
    p = gfa_put(p, t.b); *p++ = '\t';
    *p++ = t.minus ? '-' : '+'; *p++ = '\t';
    p = gfa_put(p, t.pos); *p++ = '\t';
    p = gfa_put(p, t.len2); *p++ = 'M'; *p++ = '\n';
    return p;
}

#if defined(__HIPCC__)
#include "disco_text.h"

/* ---- pieces: cut[3 r] = the first line of piece r — the first one that starts at or behind byte r * unit — cut[3 r + 1] = where it
 * starts, cut[3 r + 2] = the long reads before it (S lines of a table with two classes); r = n_pieces: the end. place has n_lines + 1
 * entries, the last one the total. A piece holds fewer than unit + GFA_MAX_LINE bytes. ---- */
__global__ void gfa_cuts_kernel(const u64 *__restrict__ place, u64 n_lines, u64 unit, u64 n_pieces, const u32 *__restrict__ ovf, u32 n_long, u64 *__restrict__ cut)
{
    u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; r <= n_pieces; r += (u64)gridDim.x * blockDim.x) {
        u64 lo = 0, hi = n_lines; /* the first index in [0, n_lines] whose place is >= r * unit */
        const u64 x = r * unit;
        while (r < n_pieces && lo < hi) {
            const u64 mid = lo + (hi - lo) / 2;
            if (place[mid] < x) lo = mid + 1;
            else hi = mid;
        }
        const u64 idx = r < n_pieces ? lo : n_lines;
        cut[3 * r] = idx;
        cut[3 * r + 1] = place[idx];
        cut[3 * r + 2] = ovf ? (idx < n_lines ? (u64)ovf[idx] : (u64)n_long) : 0ull;
    }
}

/* skip (here and in the writers below): null, or a flag per read / per edge in fetch order — a flagged one has no line (0 bytes) */
__global__ void gfa_s_measure_kernel(GfaReads g, const u8 *__restrict__ skip, u32 no_seq, u16 *__restrict__ bytes)
{
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i < g.n; i += (u64)gridDim.x * blockDim.x) bytes[i] = (skip && skip[i]) ? (u16)0 : (u16)gfa_s_bytes(gfa_name(g, i), g.len[i], no_seq != 0);
}
/* the S lines of the reads [lo, hi) into the piece that begins at byte `base` of the section: W lanes per read, lane w its word w (W =
 * the stride of the table; 8 with two classes, where the words from 8 on are gfa_s_write_long_kernel's; 1 without sequences) */
__global__ void gfa_s_write_kernel(GfaReads g, const u8 *__restrict__ skip, const u64 *__restrict__ place, u64 lo, u64 hi, u64 base, u32 no_seq, u32 W, char *__restrict__ piece)
{
    u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 total = (hi - lo) * W;
    for (; t < total; t += (u64)gridDim.x * blockDim.x) {
        const u64 i = lo + t / W;
        const u32 w = (u32)(t % W), len = g.len[i];
        if (w >= gfa_s_items(len, no_seq != 0) || (skip && skip[i])) continue;
        gfa_s_put(piece + (place[i] - base), gfa_name(g, i), len, w, no_seq ? 0ull : gfa_word(g, i, w), no_seq != 0);
    }
}
/* two classes: the words from 8 on of the long reads [jlo, jhi), SL - 8 lanes per read */
__global__ void gfa_s_write_long_kernel(GfaReads g, const u8 *__restrict__ skip, const u64 *__restrict__ place, u64 jlo, u64 jhi, u64 base, char *__restrict__ piece)
{
    u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 per = g.SL - GFA_HEAD_WORDS, total = (jhi - jlo) * per;
    for (; t < total; t += (u64)gridDim.x * blockDim.x) {
        const u64 j = jlo + t / per, i = g.long_ids[j];
        const u32 w = GFA_HEAD_WORDS + (u32)(t % per), len = g.len[i];
        if (w >= gfa_s_items(len, false) || (skip && skip[i])) continue;
        gfa_s_put(piece + (place[i] - base), gfa_name(g, i), len, w, g.full[j * g.SL + w], false);
    }
}

/* the edge in slot s, whose rank in fetch order is e; subs: substitutions by rank, or null (exact overlaps: no NM tag) */
__device__ __forceinline__ GfaL gfa_l_of(const TextView &g, const u16 *__restrict__ subs, u64 s, u64 e)
{
    const TextNumbers n = tx_numbers(g, s);
    GfaL t;
    t.a = n.a;
    t.b = n.b;
    t.orient = n.orient;
    t.ovl = n.ovl;
    t.has_nm = subs != nullptr;
    t.nm = subs ? subs[e] : 0u;
    return t;
}
__global__ void gfa_l_measure_kernel(TextView g, const u16 *__restrict__ subs, const u8 *__restrict__ skip, u8 *__restrict__ bytes)
{
    u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; s < g.n_slots; s += (u64)gridDim.x * blockDim.x) {
        if (g.valid && !g.valid[s]) continue;
        const u64 e = g.pos ? g.pos[s] : s;
        bytes[e] = (skip && skip[e]) ? (u8)0 : (u8)gfa_l_bytes(gfa_l_of(g, subs, s, e));
    }
}
/* the lines of the edges of rank [lo, hi), looked for in the slots [s_lo, s_hi) (a dense emission: the same range) */
__global__ void gfa_l_write_kernel(TextView g, const u16 *__restrict__ subs, const u8 *__restrict__ skip, const u64 *__restrict__ place, u64 s_lo, u64 s_hi, u64 lo, u64 hi, u64 base, char *__restrict__ piece)
{
    u64 s = s_lo + (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; s < s_hi; s += (u64)gridDim.x * blockDim.x) {
        if (g.valid && !g.valid[s]) continue;
        const u64 e = g.pos ? g.pos[s] : s;
        if (e < lo || e >= hi || (skip && skip[e])) continue;
        gfa_l_put(piece + (place[e] - base), gfa_l_of(g, subs, s, e));
    }
}

__device__ __forceinline__ GfaC gfa_c_of_row(const CTextView &g, u64 i)
{
    const CTextNumbers n = ctx_numbers(g, i); /* a: the contained read, b: the containing one */
    return gfa_c_of(n.b, n.a, n.orient, n.len1, n.len2, n.start);
}
__global__ void gfa_c_measure_kernel(CTextView g, u8 *__restrict__ bytes)
{
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i < g.nc; i += (u64)gridDim.x * blockDim.x) bytes[i] = (u8)gfa_c_bytes(gfa_c_of_row(g, i));
}
__global__ void gfa_c_write_kernel(CTextView g, const u64 *__restrict__ place, u64 lo, u64 hi, u64 base, char *__restrict__ piece)
{
    u64 i = lo + (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i < hi; i += (u64)gridDim.x * blockDim.x) gfa_c_put(piece + (place[i] - base), gfa_c_of_row(g, i));
}
#endif /* __HIPCC__ */

#endif /* DISCO_GFA_H_ */
