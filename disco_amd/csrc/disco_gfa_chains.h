/*
 * disco_gfa_chains.h — the compacted graph as GFA 1.0 (<prefix>.unitigs.gfa; disco_write_gfa_chains, include/disco_hip.h): every
 * composite edge of the chain contraction (disco_chains.h) is ONE segment that carries the merged sequence of the reads inside it.
 *     H \t VN:Z:1.0
 *     S \t name \t bases \t LN:i:len                every read that is neither contained nor inside a chain, in read-id order
 *     S \t c<k> \t bases \t LN:i:LN \t RC:i:m       every composite edge k, in the order of disco_fetch_chains
 *     L \t src \t so \t dst \t do \t ovl M          every edge that went into no composite edge, in the order of disco_fetch_edges
 *     L \t a \t sa \t c<k> \t + \t ovl_a M          per composite edge k its head link ...
 *     L \t c<k> \t + \t b \t sb \t ovl_b M          ... and its tail link
 * Composite edge k has the links l_0 .. l_{n-1}; its interior reads are r_j = l_j.to for j < m = n - 1, read forward iff l_j.orient & 1,
 * and r_j begins at base s_j of the segment: s_0 = 0, s_j = s_{j-1} + l_j.offset. LN = s_{m-1} + len[r_{m-1}]. Base p of the segment is
 * base p - s_j of oriented r_j for the LARGEST j with s_j <= p (with exact overlaps every read that covers p agrees; the rule says who
 * is read). sa = '+' iff l_0.orient & 2, ovl_a = len[a] - l_0.offset; sb = '+' iff l_{n-1}.orient & 1, ovl_b = len[r_{m-1}] - l_{n-1}.offset.
 *
 * The read S lines and the edge L lines are disco_gfa.h's writers behind a skip flag. The chain S section is the bulk of the file and
 * its lines have no bound (a chain can be a whole genome), so it is not cut at line ends: it is one stream of bytes, a piece is the
 * byte range [lo, hi) of it with lo a multiple of 16, and an ITEM IS 16 CONSECUTIVE BYTES OF THE STREAM, not a read. At 30x a read owns
 * about five bases, so an item per read would store five bytes at an odd address; turned round, the lane that owns bytes [P, P + 16)
 * finds the line (binary search in the scanned line starts) and the read (binary search in the scanned link offsets of that chain) that
 * hold byte P, walks on from read to read until it has its 16 characters in two registers, and stores them with ONE aligned 16-byte
 * store: a wavefront writes 1 KiB without a gap. A read that owns 32 767 bases is 2048 items on as many lanes, the clip of an item to
 * its piece is the last item's byte count, and no byte has two writers. The head "S \t c<k> \t" and the tail "\t LN:i: .. \n" of a line
 * are bytes of the stream like the bases.
 *
 * Everything up to the kernels is plain functions (host and device): disco_amd/host/gfa_chains_check.cpp runs them without a GPU.
 */
#ifndef DISCO_GFA_CHAINS_H_
#define DISCO_GFA_CHAINS_H_

#include "disco_gfa.h"

struct GfuChains {
    const disco_chain_edge *comp;
    const disco_chain_link *links;
    const uint64_t *lsum;   /* [n_links + 1]: the exclusive scan of the links' offsets; with f = first_link, s_j = lsum[f + 1 + j] - lsum[f + 1] */
    const uint64_t *cplace; /* [n_comp + 1]: where the line of composite edge k begins in the chain S section; [n_comp]: its size        */
    uint64_t n_comp;
    bool no_seq;
};

/* ---- 32 oriented bases from base q of a read ------------------------------------------------------------------------------------ */
/* forward bases [q, q + 32) of read i, MSB first (q < len; positions behind the read's last word are zero) */
GFA_HD uint64_t gfu_forward32(const GfaReads &g, uint64_t i, uint32_t len, uint32_t q)
{
    const uint32_t w = q >> 5, sh = 2u * (q & 31u), nw = (len + 31u) >> 5;
    uint64_t v = gfa_word(g, i, w) << sh;
    if (sh && w + 1 < nw) v |= gfa_word(g, i, w + 1) >> (64u - sh);
    return v;
}
/* 32 bases reversed and complemented (A0 C1 G2 T3: the complement is the bitwise one) */
GFA_HD uint64_t gfu_revcomp32(uint64_t v)
{
    v = ((v >> 2) & 0x3333333333333333ull) | ((v & 0x3333333333333333ull) << 2);
    v = ((v >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((v & 0x0F0F0F0F0F0F0F0Full) << 4);
    v = ((v >> 8) & 0x00FF00FF00FF00FFull) | ((v & 0x00FF00FF00FF00FFull) << 8);
    v = ((v >> 16) & 0x0000FFFF0000FFFFull) | ((v & 0x0000FFFF0000FFFFull) << 16);
    v = (v >> 32) | (v << 32);
    return ~v;
}
/* bases [q, q + 32) of read i as the chain reads it — forward, or its reverse complement — MSB first; what lies behind the read's
 * last base is not defined (q >= len, which no link of a true overlap asks for: nothing is read) */
GFA_HD uint64_t gfu_oriented32(const GfaReads &g, uint64_t i, uint32_t len, bool forward, uint32_t q)
{
    if (q >= len) return 0;
    if (forward) return gfu_forward32(g, i, len, q);
    const uint32_t e = len - q; /* the forward bases [e - 32, e), turned round */
    return gfu_revcomp32(e >= 32u ? gfu_forward32(g, i, len, e - 32u) : gfu_forward32(g, i, len, 0) >> (2u * (32u - e)));
}
/* the bases [8 k, 8 k + 8) of a word as characters, the first one in the low byte */
GFA_HD uint64_t gfu_chars8(uint64_t word, uint32_t k)
{
    uint64_t v = 0;
    for (int b = 0; b < 8; b++) {
        const uint32_t code = (uint32_t)(word >> (62 - 2 * (8 * (int)k + b))) & 3u;
        v |= (uint64_t)((0x54474341u >> (8 * code)) & 0xFFu) << (8 * b); /* A C G T */
    }
    return v;
}

/* ---- the line of a composite edge ------------------------------------------------------------------------------------------------- */
struct GfuLine {
    uint64_t first, m; /* its first link; its interior reads (RC) */
    uint64_t LN, body; /* bases; characters between the tabs (1 without sequences) */
    uint64_t bytes;
    uint32_t pre; /* S \t c k \t */
};
GFA_HD GfuLine gfu_line(const GfuChains &h, const uint16_t *len, uint64_t k)
{
    GfuLine t;
    t.first = h.comp[k].first_link;
    t.m = (uint64_t)h.comp[k].n_links - 1;
    t.LN = h.lsum[t.first + t.m] - h.lsum[t.first + 1] + len[h.links[t.first + t.m - 1].to];
    t.body = h.no_seq ? 1 : t.LN;
    t.pre = 4u + gfa_digits(k);
    /* \t LN:i: LN \t RC:i: m \n : 13 fixed characters */
    t.bytes = t.pre + t.body + 13u + gfa_digits(t.LN) + gfa_digits(t.m);
    return t;
}
/* digit i, from the left, of a number of d digits */
GFA_HD char gfu_digit(uint64_t v, uint32_t d, uint32_t i)
{
    for (uint32_t t = d - 1 - i; t > 0; t--) v /= 10;
    return (char)('0' + (uint32_t)(v % 10));
}
GFA_HD char gfu_head_char(uint64_t k, uint32_t pre, uint32_t o) { return o == 0 ? 'S' : (o == 1 || o + 1 == pre) ? '\t' : o == 2 ? 'c' : gfu_digit(k, pre - 4u, o - 3u); }
GFA_HD char gfu_tail_char(uint64_t LN, uint64_t m, uint32_t o)
{
    const uint32_t dl = gfa_digits(LN), dm = gfa_digits(m);
    if (o < 6) return (char)(0x3A693A4E4C09ull >> (8 * o)); /* \t L N : i : */
    o -= 6;
    if (o < dl) return gfu_digit(LN, dl, o);
    o -= dl;
    if (o < 6) return (char)(0x3A693A435209ull >> (8 * o)); /* \t R C : i : */
    o -= 6;
    return o < dm ? gfu_digit(m, dm, o) : '\n';
}

/* ---- an item: 16 bytes of the chain S section ---------------------------------------------------------------------------------- */
struct GfuAcc {
    uint64_t lo, hi; /* character i is byte i & 7 of lo (i < 8) or hi */
    uint32_t n;
};
/* cnt <= 8 characters behind the n that are there (n + cnt <= 16) */
GFA_HD void gfu_push(GfuAcc &a, uint64_t c8, uint32_t cnt)
{
    if (cnt == 0) return;
    if (cnt < 8) c8 &= (1ull << (8 * cnt)) - 1;
    const uint32_t sh = 8u * (a.n & 7u);
    if (a.n < 8) {
        a.lo |= c8 << sh;
        if (sh) a.hi |= c8 >> (64u - sh);
    } else a.hi |= c8 << sh;
    a.n += cnt;
}
/* the bytes [P, P + nb) of the section, nb <= 16 and inside it */
GFA_HD GfuAcc gfu_bytes16(const GfaReads &g, const GfuChains &h, uint64_t P, uint32_t nb)
{
    GfuAcc a;
    a.lo = a.hi = 0;
    a.n = 0;
    uint64_t lo = 0, hi = h.n_comp; /* the first line that begins behind P; the one before it holds P */
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (h.cplace[mid] <= P) lo = mid + 1;
        else hi = mid;
    }
    uint64_t k = lo - 1;
    while (a.n < nb) {
        const GfuLine t = gfu_line(h, g.len, k);
        uint64_t o = P + a.n - h.cplace[k];
        for (; o < t.pre && a.n < nb; o++) gfu_push(a, (uint64_t)(uint8_t)gfu_head_char(k, t.pre, (uint32_t)o), 1);
        if (a.n < nb && o < t.pre + t.body) {
            if (h.no_seq) {
                gfu_push(a, '*', 1);
                o++;
            } else {
                uint64_t p = o - t.pre;
                const uint64_t *s = h.lsum + t.first + 1; /* s_j = s[j] - s[0] */
                uint64_t jl = 0, jh = t.m;                /* the first read that begins behind p; the one before it owns p */
                while (jl < jh) {
                    const uint64_t mid = jl + (jh - jl) / 2;
                    if (s[mid] - s[0] <= p) jl = mid + 1;
                    else jh = mid;
                }
                uint64_t j = jl - 1;
                while (a.n < nb && p < t.LN) {
                    const uint64_t sj = s[j] - s[0], end = j + 1 < t.m ? s[j + 1] - s[0] : t.LN;
                    if (end > p) {
                        const disco_chain_link l = h.links[t.first + j];
                        const uint64_t left = end - p;
                        const uint32_t cnt = left < nb - a.n ? (uint32_t)left : nb - a.n;
                        const uint64_t word = gfu_oriented32(g, l.to, g.len[l.to], (l.orient & 1u) != 0, (uint32_t)(p - sj));
                        gfu_push(a, gfu_chars8(word, 0), cnt < 8 ? cnt : 8u);
                        if (cnt > 8) gfu_push(a, gfu_chars8(word, 1), cnt - 8u);
                        p += cnt;
                    }
                    if (p >= end) j++;
                }
                o = t.pre + p;
            }
        }
        for (; o < t.bytes && a.n < nb; o++) gfu_push(a, (uint64_t)(uint8_t)gfu_tail_char(t.LN, t.m, (uint32_t)(o - t.pre - t.body)), 1);
        if (o == t.bytes) k++;
    }
    return a;
}
/* item t of the piece that holds the bytes [lo, hi) of the section (lo a multiple of 16, piece 16-byte aligned): one store of 16 bytes,
 * narrower ones at the ragged end of the piece */
GFA_HD void gfu_item(const GfaReads &g, const GfuChains &h, uint64_t lo, uint64_t hi, uint64_t t, char *piece)
{
    const uint64_t P = lo + 16 * t;
    const uint32_t nb = hi - P < 16 ? (uint32_t)(hi - P) : 16u;
    const GfuAcc a = gfu_bytes16(g, h, P, nb);
    GfaChunk c;
    c.q[0] = a.lo;
    c.q[1] = a.hi;
    c.q[2] = c.q[3] = 0;
    gfa_store(piece + 16 * t, c, nb);
}
GFA_HD uint64_t gfu_items(uint64_t lo, uint64_t hi) { return (hi - lo + 15) >> 4; }

/* ---- the two L lines of a composite edge ------------------------------------------------------------------------------------------ */
struct GfuL {
    uint64_t a, b, k; /* names of the two end reads */
    uint32_t a_plus, b_plus, ovl_a, ovl_b;
};
GFA_HD GfuL gfu_l_of(const GfaReads &g, const GfuChains &h, uint64_t k)
{
    const disco_chain_edge c = h.comp[k];
    const disco_chain_link l0 = h.links[c.first_link], ln = h.links[c.first_link + c.n_links - 1];
    GfuL t;
    t.a = gfa_name(g, c.a);
    t.b = gfa_name(g, c.b);
    t.k = k;
    t.a_plus = (l0.orient >> 1) & 1u;
    t.b_plus = ln.orient & 1u;
    t.ovl_a = g.len[c.a] - l0.offset;
    t.ovl_b = g.len[h.links[c.first_link + c.n_links - 2].to] - ln.offset;
    return t;
}
GFA_HD uint32_t gfu_l_bytes(const GfuL &t)
{
    /* L \t a \t s \t c k \t + \t ovl M \n : 11 fixed characters, and the same 11 in the tail link */
    return gfa_digits(t.a) + gfa_digits(t.b) + 2u * gfa_digits(t.k) + gfa_digits(t.ovl_a) + gfa_digits(t.ovl_b) + 22u;
}
GFA_HD char *gfu_l_put(char *p, const GfuL &t)
{
    *p++ = 'L'; *p++ = '\t';
    p = gfa_put(p, t.a); *p++ = '\t';
    *p++ = t.a_plus ? '+' : '-'; *p++ = '\t'; *p++ = 'c';
    p = gfa_put(p, t.k); *p++ = '\t'; *p++ = '+'; *p++ = '\t';
    p = gfa_put(p, t.ovl_a); *p++ = 'M'; *p++ = '\n';
    *p++ = 'L'; *p++ = '\t'; *p++ = 'c';
    p = gfa_put(p, t.k); *p++ = '\t'; *p++ = '+'; *p++ = '\t';
    p = gfa_put(p, t.b); *p++ = '\t';
    *p++ = t.b_plus ? '+' : '-'; *p++ = '\t';
    p = gfa_put(p, t.ovl_b); *p++ = 'M'; *p++ = '\n';
    return p;
}

#if defined(__HIPCC__)
/* ---- which reads keep a line of their own: skip[i] = 1 for a contained read and for a read inside a chain. Every link's target is
 * marked; the last link of a composite edge ends at its b, which is no inner node of any chain (a chain ends where a node cannot be
 * absorbed) and gets its contained flag back ---- */
__global__ void gfu_mark_links_kernel(const disco_chain_link *__restrict__ links, u64 n_links, u8 *__restrict__ skip)
{
    u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; x < n_links; x += (u64)gridDim.x * blockDim.x) skip[links[x].to] = 1;
}
__global__ void gfu_unmark_ends_kernel(const disco_chain_edge *__restrict__ comp, u64 n_comp, const u8 *__restrict__ contained, u8 *__restrict__ skip)
{
    u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; k < n_comp; k += (u64)gridDim.x * blockDim.x) skip[comp[k].b] = contained[comp[k].b];
}
__global__ void gfu_link_offsets_kernel(const disco_chain_link *__restrict__ links, u64 n_links, u32 *__restrict__ off)
{
    u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; x < n_links; x += (u64)gridDim.x * blockDim.x) off[x] = links[x].offset;
}
/* bytes of every composite edge's S line (h.cplace is not looked at) */
__global__ void gfu_s_measure_kernel(GfuChains h, const u16 *__restrict__ len, u64 *__restrict__ bytes)
{
    u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; k < h.n_comp; k += (u64)gridDim.x * blockDim.x) bytes[k] = gfu_line(h, len, k).bytes;
}
/* THE SPELLING KERNEL: the bytes [lo, hi) of the chain S section into the piece, a lane per 16 of them */
__global__ void __launch_bounds__(256) gfu_spell_kernel(GfaReads g, GfuChains h, u64 lo, u64 hi, char *__restrict__ piece)
{
    u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 total = gfu_items(lo, hi);
    for (; t < total; t += (u64)gridDim.x * blockDim.x) gfu_item(g, h, lo, hi, t, piece);
}
__global__ void gfu_l_measure_kernel(GfaReads g, GfuChains h, u8 *__restrict__ bytes)
{
    u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; k < h.n_comp; k += (u64)gridDim.x * blockDim.x) bytes[k] = (u8)gfu_l_bytes(gfu_l_of(g, h, k));
}
__global__ void gfu_l_write_kernel(GfaReads g, GfuChains h, const u64 *__restrict__ place, u64 lo, u64 hi, u64 base, char *__restrict__ piece)
{
    u64 k = lo + (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; k < hi; k += (u64)gridDim.x * blockDim.x) gfu_l_put(piece + (place[k] - base), gfu_l_of(g, h, k));
}
#endif /* __HIPCC__ */

#endif /* DISCO_GFA_CHAINS_H_ */
