/*
 * disco_partext.h — the lines of <prefix>_<t>_ParSimpleEdges.txt formatted on the GPU (printEdge, SG/OverlapGraphSimple.cpp:658-690;
 * disco_amd/host/parsimple.h):
 *     src \t dst \t orient,offset,offset+len(dst),0,0 \t (read,orientation bit,offset)(…)… \n              source <= destination
 * A final edge of the partial simplification is described by the host pass as a short list of PIECES (disco_ps_piece): an inline link,
 * or all links of a composite edge the device contracted (disco_chains.h), forward or reversed. The links themselves never leave the
 * device: a lane is one ITEM of a line — item 0 of an edge is its header, item j >= 1 the inner read behind the edge's link j - 1 (the
 * last link leads to the destination and prints nothing) — finds its edge and its piece by binary search in two prefix tables (items
 * per edge, links per piece: as many entries as the description has edges and pieces), resolves its link and measures or writes its
 * few bytes. Measure -> scan -> write, as for the edge and contained lines (disco_text.h). The newline belongs to the edge's last item.
 *
 * Item resolution and formatting are plain functions (host and device), so the same code is exercised without a GPU by
 * disco_amd/host/partext_check.cpp; the kernels at the end need hipcc. (ps_digits / ps_put are tx_digits / tx_put of disco_text.h,
 * repeated here because that header is device-only.)
 */
#ifndef DISCO_PARTEXT_H_
#define DISCO_PARTEXT_H_

#include <stdint.h>

#include "../../include/disco_hip.h"

#if defined(__HIPCC__)
#define PS_HD __host__ __device__ __forceinline__
#else
#define PS_HD inline
#endif

struct PsView {
    const disco_ps_edge *edges;     /* [n_edges] in printing direction, in the files' line order                     */
    const disco_ps_piece *pieces;   /* [n_pieces]                                                                    */
    const uint64_t *edge_item;      /* [n_edges + 1] items before edge e (an edge of L links has L items)            */
    const uint64_t *piece_link;     /* [n_pieces + 1] links before piece p                                           */
    const disco_chain_edge *comp;   /* the device's composite edges and their links (disco_contract_chains)          */
    const disco_chain_link *links;
    const uint16_t *len;            /* read length by id                                                             */
    const uint64_t *file_index;     /* [n] or null: id + 1                                                           */
    uint64_t n_edges, n_pieces, n_items;
};

PS_HD uint32_t ps_twin(uint32_t o) { return ((o >> 1) ^ 1u) | (((o & 1u) ^ 1u) << 1); } /* get_twin_orient, SG/EdgeSimple.cpp:277 */
PS_HD uint32_t ps_digits(uint64_t v)
{
    uint32_t d = 1;
    while (v >= 10) {
        v /= 10;
        d++;
    }
    return d;
}
PS_HD char *ps_put(char *p, uint64_t v)
{
    const uint32_t d = ps_digits(v);
    for (uint32_t i = d; i-- > 0;) {
        p[i] = (char)('0' + (uint32_t)(v % 10));
        v /= 10;
    }
    return p + d;
}
/* the last index in t[lo .. hi) whose value is <= x (t ascending, t[lo] <= x) */
PS_HD uint64_t ps_find(const uint64_t *t, uint64_t lo, uint64_t hi, uint64_t x)
{
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (t[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

struct PsLink {
    uint32_t to, offset, orient;
};
/* link r of piece p in the piece's direction. A reversed composite with links l_0 .. l_{m-1} out of node A contributes, for
 * j = m-1 .. 0, {to = from_j, offset = len[l_j.to] + l_j.offset - len[from_j], orient = twin(l_j.orient)}, from_j = l_{j-1}.to, from_0 = A
 * (Graph::append_links of parsimple.cpp) */
PS_HD PsLink ps_link(const PsView &g, const disco_ps_piece &p, uint64_t r)
{
    PsLink o;
    if (p.kind == 0) {
        o.to = p.a;
        o.offset = p.offset;
        o.orient = p.orient;
        return o;
    }
    const disco_chain_edge ce = g.comp[p.a];
    if (p.kind == 1) {
        const disco_chain_link l = g.links[ce.first_link + r];
        o.to = l.to;
        o.offset = l.offset;
        o.orient = l.orient;
        return o;
    }
    const uint64_t j = ce.n_links - 1 - r;
    const disco_chain_link l = g.links[ce.first_link + j];
    const uint32_t from = j ? g.links[ce.first_link + j - 1].to : (uint32_t)ce.a;
    o.to = from;
    o.offset = (uint32_t)((int64_t)g.len[l.to] + (int64_t)l.offset - (int64_t)g.len[from]);
    o.orient = ps_twin(l.orient);
    return o;
}

struct PsItem { /* what one lane prints */
    uint64_t a, b;    /* header: the file indices of source and destination; inner read: a = its file index */
    uint32_t orient, offset, end;
    bool header, last;
};
PS_HD PsItem ps_item(const PsView &g, uint64_t i)
{
    PsItem t;
    const uint64_t e = ps_find(g.edge_item, 0, g.n_edges, i), j = i - g.edge_item[e];
    const disco_ps_edge x = g.edges[e];
    t.header = j == 0;
    t.last = i + 1 == g.edge_item[e + 1];
    if (t.header) {
        t.a = g.file_index ? g.file_index[x.src] : x.src + 1;
        t.b = g.file_index ? g.file_index[x.dst] : x.dst + 1;
        t.orient = x.orient;
        t.offset = (uint32_t)x.offset;
        t.end = (uint32_t)x.offset + g.len[x.dst];
        return t;
    }
    const uint64_t q = g.piece_link[x.first_piece] + (j - 1);
    const uint64_t p = ps_find(g.piece_link, x.first_piece, x.first_piece + x.n_pieces, q);
    const PsLink l = ps_link(g, g.pieces[p], q - g.piece_link[p]);
    t.a = g.file_index ? g.file_index[l.to] : (uint64_t)l.to + 1;
    t.b = 0;
    t.orient = l.orient & 1u;
    t.offset = l.offset;
    t.end = 0;
    return t;
}
PS_HD uint32_t ps_item_bytes(const PsItem &t)
{
    /* header: a \t b \t o , offset , end ,0,0 \t : 9 fixed characters + the orientation digit; inner read: ( a , o , offset ) : 4 + the bit */
    const uint32_t body = t.header ? ps_digits(t.a) + ps_digits(t.b) + ps_digits(t.offset) + ps_digits(t.end) + 10 : ps_digits(t.a) + ps_digits(t.offset) + 5;
    return body + (t.last ? 1u : 0u);
}
PS_HD char *ps_put_item(char *p, const PsItem &t)
{
    if (t.header) {
        p = ps_put(p, t.a); *p++ = '\t';
        p = ps_put(p, t.b); *p++ = '\t';
        *p++ = (char)('0' + t.orient); *p++ = ',';
        p = ps_put(p, t.offset); *p++ = ',';
        p = ps_put(p, t.end); *p++ = ','; *p++ = '0'; *p++ = ','; *p++ = '0'; *p++ = '\t';
    } else {
        *p++ = '(';
        p = ps_put(p, t.a); *p++ = ',';
        *p++ = (char)('0' + t.orient); *p++ = ',';
        p = ps_put(p, t.offset); *p++ = ')';
    }
    if (t.last) *p++ = '\n';
    return p;
}

#if defined(__HIPCC__)
__global__ void ptext_measure_kernel(PsView g, unsigned char *__restrict__ bytes)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i < g.n_items; i += (uint64_t)gridDim.x * blockDim.x) bytes[i] = (unsigned char)ps_item_bytes(ps_item(g, i));
}
/* first byte of every file: the place of the first item of the first edge it holds (first_item[t], n_items where no edge follows;
 * place has n_items + 1 entries, the last one the total) */
__global__ void ptext_offsets_kernel(const uint64_t *__restrict__ first_item, const unsigned long long *__restrict__ place, uint32_t n_files, uint64_t *__restrict__ off)
{
    uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; t <= n_files; t += (uint64_t)gridDim.x * blockDim.x) off[t] = place[first_item[t]];
}
__global__ void ptext_write_kernel(PsView g, const unsigned long long *__restrict__ place, char *__restrict__ text)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i < g.n_items; i += (uint64_t)gridDim.x * blockDim.x) ps_put_item(text + place[i], ps_item(g, i));
}
#endif

#endif /* DISCO_PARTEXT_H_ */
