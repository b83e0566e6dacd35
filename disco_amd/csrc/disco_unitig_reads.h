/*
 * disco_unitig_reads.h — where every read lies in the compacted graph (<prefix>.unitigs.reads; disco_write_unitig_reads,
 * include/disco_hip.h): the layout behind <prefix>.unitigs.gfa (disco_gfa_chains.h), contained reads and chain interiors included.
 *     H \t unitig-reads \t 1
 *     U \t segment \t LN \t reads \t bases                              one per S line of <prefix>.unitigs.gfa, in that file's order
 *     R \t read \t segment \t strand \t start \t len \t root \t hops    one per read, in read-id order
 * The statement of an R line: bases [start, start + len) of the segment's S line are the read, or its reverse complement for '-'.
 *
 * ROOTS. A contained read x carries the key of its direct container y, which may be contained itself. A state is ONE 64-bit word per
 * read — ancestor (31 bits) | position in the ancestor (15) | minus (1) | hops (17) — "oriented x is ancestor[pos, pos + len[x]), on the
 * ancestor's strand unless minus". It begins as (x, 0, plus, 0) or as the decoded key (y, p, minus, 1), and two states compose: x at
 * (pos, s) of y and y at (q, t) of z give x at q + pos, s of z when t is plus and at q + len[y] - pos - len[x], !s when t is minus. The
 * composition is associative, so the roots are found by pointer doubling: a round replaces every state by its composition with its
 * ancestor's state, between two arrays, and the rounds end when one moves nobody. A hop lengthens the read or keeps its length and
 * lowers the id, and two hops of equal length cannot follow each other, so a nest is less than 2^16 deep: UTR_MAX_ROUNDS rounds settle
 * every set of keys that has no cycle, and one that has not settled by then is refused.
 *
 * SEGMENTS. A root that is interior read r_j of composite edge k lies on c<k> at s_j, forward iff l_j.orient & 1 (a lane per link
 * scatters that to the read); every other root is its own segment. The last step is the same composition with (s_j, forward).
 *
 * COUNTS. A lane per read adds 1 and its length to its root's counters: one atomic per read, spread over the roots as the keys are
 * spread over the containers. A chain's totals take none: the interior reads' counters are gathered in link order (0 for a chain's
 * last link), scanned, and the chain's total is the difference over its links — a chain can be a genome, and an atomic per read on one
 * address is what that would cost.
 *
 * Everything up to the kernels is plain functions (host and device): disco_amd/host/unitig_reads_check.cpp runs them without a GPU.
 */
#ifndef DISCO_UNITIG_READS_H_
#define DISCO_UNITIG_READS_H_

#include "disco_gfa_chains.h"

#define UTR_HEADER "H\tunitig-reads\t1\n"
#define UTR_MAX_ROUNDS 17u
#define UTR_NO_CHAIN 0xFFFFFFFFu /* cseg of a read that is no interior read of a composite edge */

/* ---- the state word ---------------------------------------------------------------------------------------------------------------- */
struct UtrState {
    uint64_t anc;
    uint32_t pos, minus, hops;
};
/* (fields are cut to their widths: what a cycle or a key that names no read makes of them must not reach a neighbour) */
GFA_HD uint64_t utr_pack(const UtrState &s)
{
    return ((s.anc & 0x7FFFFFFFull) << 33) | ((uint64_t)(s.pos & 0x7FFFu) << 18) | ((uint64_t)(s.minus & 1u) << 17) | (uint64_t)(s.hops > 0x1FFFFu ? 0x1FFFFu : s.hops);
}
GFA_HD UtrState utr_unpack(uint64_t w)
{
    UtrState s;
    s.anc = w >> 33;
    s.pos = (uint32_t)(w >> 18) & 0x7FFFu;
    s.minus = (uint32_t)(w >> 17) & 1u;
    s.hops = (uint32_t)w & 0x1FFFFu;
    return s;
}
GFA_HD UtrState utr_self(uint64_t x)
{
    UtrState s;
    s.anc = x;
    s.pos = s.minus = s.hops = 0;
    return s;
}
/* a contained row's numbers (disco_contained_row: container y, orient, start): what gfa_c_of makes of them, as a state of one hop */
GFA_HD UtrState utr_of_row(uint64_t y, uint32_t orient, uint32_t start, uint32_t len_y, uint32_t len_x)
{
    const GfaC t = gfa_c_of(y, 0, orient, len_y, len_x, start);
    UtrState s;
    s.anc = y;
    s.pos = t.pos;
    s.minus = t.minus;
    s.hops = 1;
    return s;
}
/* x (len_x bases) at s of y = s.anc (len_y bases), y at t of z = t.anc: x in z */
GFA_HD UtrState utr_compose(const UtrState &s, const UtrState &t, uint32_t len_y, uint32_t len_x)
{
    UtrState r;
    r.anc = t.anc;
    r.pos = t.minus ? t.pos + len_y - s.pos - len_x : t.pos + s.pos;
    r.minus = t.minus ? s.minus ^ 1u : s.minus;
    r.hops = s.hops + t.hops;
    return r;
}
/* a root's state: itself, no hop (a read on a cycle of 2^r keys comes back to itself too, with hops: it is no root and never settles) */
GFA_HD bool utr_is_root(const UtrState &t, uint64_t id) { return t.anc == id && t.hops == 0; }
/* one round of the doubling for read x: -> 1 when it moved */
GFA_HD uint32_t utr_round(const uint64_t *cur, uint64_t *next, const uint16_t *len, uint64_t x)
{
    const uint64_t w = cur[x];
    const UtrState s = utr_unpack(w), t = utr_unpack(cur[s.anc]);
    if (utr_is_root(t, s.anc)) { /* the ancestor is a root (or x is one) */
        next[x] = w;
        return 0;
    }
    next[x] = utr_pack(utr_compose(s, t, len[s.anc], len[x]));
    return 1;
}

/* ---- a link's composite edge: the last k with first_link <= x (first_link is the running sum of n_links) ---------------------------- */
GFA_HD uint64_t utr_chain_of_link(const GfuChains &h, uint64_t x)
{
    uint64_t lo = 0, hi = h.n_comp;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (h.comp[mid].first_link <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}
/* link x: is its target an interior read of its composite edge k (every link but the last)? */
GFA_HD bool utr_link_interior(const GfuChains &h, uint64_t x, uint64_t *k)
{
    *k = utr_chain_of_link(h, x);
    return x + 1 < h.comp[*k].first_link + h.comp[*k].n_links;
}
/* the place of an interior link's read: cseg = k | forward << 31, cpos = s_j */
GFA_HD void utr_place_link(const GfuChains &h, uint64_t x, uint32_t *cseg, uint64_t *cpos)
{
    uint64_t k;
    if (!utr_link_interior(h, x, &k)) return;
    const disco_chain_link l = h.links[x];
    cseg[l.to] = (uint32_t)k | ((l.orient & 1u) << 31);
    cpos[l.to] = h.lsum[x + 1] - h.lsum[h.comp[k].first_link + 1];
}

/* ---- everything the lines are made from ------------------------------------------------------------------------------------------ */
struct UtrView {
    const uint64_t *state; /* [n] settled: the ancestor is the root */
    const uint32_t *cseg;  /* [n] */
    const uint64_t *cpos;  /* [n] */
    const uint32_t *rcnt;  /* [n] reads whose root this read is (itself included) */
    const uint64_t *rbases; /* [n] ... and their bases */
    const uint64_t *kcnt, *kbases; /* [n_links + 1]: exclusive scans of the interior reads' counters in link order */
};
struct UtrR {
    uint64_t read, root, seg, start; /* names; seg: a read's name or k */
    uint32_t on_chain, minus, len, hops;
};
GFA_HD UtrR utr_r_of(const GfaReads &g, const UtrView &v, uint64_t x)
{
    const UtrState s = utr_unpack(v.state[x]);
    const uint32_t c = v.cseg[s.anc];
    UtrR t;
    t.read = gfa_name(g, x);
    t.root = gfa_name(g, s.anc);
    t.len = g.len[x];
    t.hops = s.hops;
    t.on_chain = c != UTR_NO_CHAIN;
    if (t.on_chain) {
        const bool forward = (c >> 31) != 0;
        t.seg = c & 0x7FFFFFFFu;
        t.start = forward ? v.cpos[s.anc] + s.pos : v.cpos[s.anc] + g.len[s.anc] - s.pos - t.len;
        t.minus = forward ? s.minus : s.minus ^ 1u;
    } else {
        t.seg = t.root;
        t.start = s.pos;
        t.minus = s.minus;
    }
    return t;
}
GFA_HD uint32_t utr_r_bytes(const UtrR &t)
{
    /* R \t read \t [c] seg \t s \t start \t len \t root \t hops \n : 10 fixed characters */
    return gfa_digits(t.read) + t.on_chain + gfa_digits(t.seg) + gfa_digits(t.start) + gfa_digits(t.len) + gfa_digits(t.root) + gfa_digits(t.hops) + 10u;
}
GFA_HD char *utr_r_put(char *p, const UtrR &t)
{
    *p++ = 'R'; *p++ = '\t';
    p = gfa_put(p, t.read); *p++ = '\t';
    if (t.on_chain) *p++ = 'c';
    p = gfa_put(p, t.seg); *p++ = '\t';
    *p++ = t.minus ? '-' : '+'; *p++ = '\t';
    p = gfa_put(p, t.start); *p++ = '\t';
    p = gfa_put(p, t.len); *p++ = '\t';
    p = gfa_put(p, t.root); *p++ = '\t';
    p = gfa_put(p, t.hops); *p++ = '\n';
    return p;
}

struct UtrU {
    uint64_t seg, LN, reads, bases;
    uint32_t on_chain;
};
GFA_HD UtrU utr_u_of_read(const GfaReads &g, const UtrView &v, uint64_t i)
{
    UtrU t;
    t.seg = gfa_name(g, i);
    t.LN = g.len[i];
    t.reads = v.rcnt[i];
    t.bases = v.rbases[i];
    t.on_chain = 0;
    return t;
}
GFA_HD UtrU utr_u_of_chain(const GfaReads &g, const GfuChains &h, const UtrView &v, uint64_t k)
{
    const uint64_t f = h.comp[k].first_link, e = f + h.comp[k].n_links;
    UtrU t;
    t.seg = k;
    t.LN = gfu_line(h, g.len, k).LN;
    t.reads = v.kcnt[e] - v.kcnt[f];
    t.bases = v.kbases[e] - v.kbases[f];
    t.on_chain = 1;
    return t;
}
GFA_HD uint32_t utr_u_bytes(const UtrU &t)
{
    /* U \t [c] seg \t LN \t reads \t bases \n : 6 fixed characters */
    return t.on_chain + gfa_digits(t.seg) + gfa_digits(t.LN) + gfa_digits(t.reads) + gfa_digits(t.bases) + 6u;
}
GFA_HD char *utr_u_put(char *p, const UtrU &t)
{
    *p++ = 'U'; *p++ = '\t';
    if (t.on_chain) *p++ = 'c';
    p = gfa_put(p, t.seg); *p++ = '\t';
    p = gfa_put(p, t.LN); *p++ = '\t';
    p = gfa_put(p, t.reads); *p++ = '\t';
    p = gfa_put(p, t.bases); *p++ = '\n';
    return p;
}

#if defined(__HIPCC__)
enum { UTR_BAD_KEYS = 0, UTR_CTRS = 1 };
/* the initial states. A key that names no read must not index anything: counted, the read left as its own root, and the caller fails */
__global__ void utr_init_kernel(const u64 *__restrict__ best, const u8 *__restrict__ contained, const u16 *__restrict__ len, u64 n, u32 k, uint64_t *__restrict__ state,
                                u32 *__restrict__ ctr)
{
    u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; x < n; x += (u64)gridDim.x * blockDim.x) {
        UtrState s = utr_self(x);
        if (contained[x]) {
            const u64 key = best[x], y = CKEY_SUPER(key);
            if (y < n) {
                u32 orient, start;
                disco_map_hit(CKEY_SUFFIX(key), CKEY_REV(key), len[y], k, CKEY_J(key), &orient, &start);
                s = utr_of_row(y, orient, start, len[y], len[x]);
            } else atomicAdd(&ctr[UTR_BAD_KEYS], 1u);
        }
        state[x] = utr_pack(s);
    }
}
/* one round; moved: this round's flag (every lane that moved stores the same 1) */
__global__ void utr_round_kernel(const uint64_t *__restrict__ cur, uint64_t *__restrict__ next, const u16 *__restrict__ len, u64 n, u32 *__restrict__ moved)
{
    u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; x < n; x += (u64)gridDim.x * blockDim.x)
        if (utr_round(cur, next, len, x)) *moved = 1u;
}
__global__ void utr_place_links_kernel(GfuChains h, u64 n_links, u32 *__restrict__ cseg, uint64_t *__restrict__ cpos)
{
    u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; x < n_links; x += (u64)gridDim.x * blockDim.x) utr_place_link(h, x, cseg, cpos);
}
/* every read to its root's counters */
__global__ void utr_count_kernel(const uint64_t *__restrict__ state, const u16 *__restrict__ len, u64 n, u32 *__restrict__ rcnt, u64 *__restrict__ rbases)
{
    u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; x < n; x += (u64)gridDim.x * blockDim.x) {
        const u64 r = utr_unpack(state[x]).anc;
        atomicAdd(&rcnt[r], 1u);
        atomicAdd(&rbases[r], (u64)len[x]);
    }
}
/* the interior reads' counters in link order, 0 for the last link of a composite edge */
__global__ void utr_gather_kernel(GfuChains h, u64 n_links, const u32 *__restrict__ rcnt, const u64 *__restrict__ rbases, u32 *__restrict__ lcnt, u64 *__restrict__ lbases)
{
    u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; x < n_links; x += (u64)gridDim.x * blockDim.x) {
        uint64_t k;
        const bool in = utr_link_interior(h, x, &k);
        const u32 r = h.links[x].to;
        lcnt[x] = in ? rcnt[r] : 0u;
        lbases[x] = in ? rbases[r] : 0ull;
    }
}
/* U lines of the read segments, behind the skip flags of the S lines of <prefix>.unitigs.gfa */
__global__ void utr_u_read_measure_kernel(GfaReads g, UtrView v, const u8 *__restrict__ skip, u8 *__restrict__ bytes)
{
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i < g.n; i += (u64)gridDim.x * blockDim.x) bytes[i] = skip[i] ? (u8)0 : (u8)utr_u_bytes(utr_u_of_read(g, v, i));
}
__global__ void utr_u_read_write_kernel(GfaReads g, UtrView v, const u8 *__restrict__ skip, const u64 *__restrict__ place, u64 lo, u64 hi, u64 base, char *__restrict__ piece)
{
    u64 i = lo + (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i < hi; i += (u64)gridDim.x * blockDim.x)
        if (!skip[i]) utr_u_put(piece + (place[i] - base), utr_u_of_read(g, v, i));
}
__global__ void utr_u_chain_measure_kernel(GfaReads g, GfuChains h, UtrView v, u8 *__restrict__ bytes)
{
    u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; k < h.n_comp; k += (u64)gridDim.x * blockDim.x) bytes[k] = (u8)utr_u_bytes(utr_u_of_chain(g, h, v, k));
}
__global__ void utr_u_chain_write_kernel(GfaReads g, GfuChains h, UtrView v, const u64 *__restrict__ place, u64 lo, u64 hi, u64 base, char *__restrict__ piece)
{
    u64 k = lo + (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; k < hi; k += (u64)gridDim.x * blockDim.x) utr_u_put(piece + (place[k] - base), utr_u_of_chain(g, h, v, k));
}
__global__ void utr_r_measure_kernel(GfaReads g, UtrView v, u8 *__restrict__ bytes)
{
    u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; x < g.n; x += (u64)gridDim.x * blockDim.x) bytes[x] = (u8)utr_r_bytes(utr_r_of(g, v, x));
}
__global__ void utr_r_write_kernel(GfaReads g, UtrView v, const u64 *__restrict__ place, u64 lo, u64 hi, u64 base, char *__restrict__ piece)
{
    u64 x = lo + (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; x < hi; x += (u64)gridDim.x * blockDim.x) utr_r_put(piece + (place[x] - base), utr_r_of(g, v, x));
}
#endif /* __HIPCC__ */

#endif /* DISCO_UNITIG_READS_H_ */
