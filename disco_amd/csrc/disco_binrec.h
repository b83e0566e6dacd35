/*
 * disco_binrec.h — the records of the binary side output formed on the GPU (layout: include/disco_hip.h
 * disco_bin_edge / disco_bin_contained, disco_amd/host/writer.h; the same content as saveParGraphToFile's lines, BG/OverlapGraph.cpp:808-867,
 * and the contained-read lines, :438-447, without the formatting on this side and the parsing on the consumer's).
 * Fixed records of 40 bytes: record i of a kind lies at byte 40 i, so nothing is measured or scanned — one lane per record reads what
 * the text kernels read (disco_text.h tx_numbers / ctx_numbers), builds the record in registers as five 64-bit words and stores those.
 * Every byte of a record is written (the pads as zeros): a piece buffer never holds bytes the kernel did not put there, and records are
 * 8-byte aligned because the piece buffers are. The records [lo, hi) of a kind go to piece[0 .. 40 (hi - lo)).
 * No variant that stages a wave's records in LDS to store them as contiguous lines: the kernels are not what the stage waits for
 * (profiles/binary_records.txt; profiles/par_simple_text.txt records the same decision for ptext_write_kernel).
 */
#ifndef DISCO_BINREC_H_
#define DISCO_BINREC_H_

#include "disco_text.h"

#define BINREC_WORDS 5 /* 40 bytes */

struct BinEdgeView {
    const u64 *src64; /* the emission's sources where it is dense (slot i is edge i) ... */
    const u32 *src32; /* ... or the compacted ones (emit_compact32_kernel); exactly one of the two is set */
    const u64 *ent;   /* the entries of the same slots */
    const u16 *len;
    const u64 *file_index; /* [n] or null: id + 1 */
    const u16 *edge_file;  /* [ne] or null: file 0 */
    const u16 *subs;       /* [ne] or null: 0 (exact overlaps) */
    u32 n_files;
};

/* little endian: the first of two 32-bit fields is the low half of their word */
__host__ __device__ __forceinline__ u64 binrec_pair(u32 first, u32 second) { return (u64)first | ((u64)second << 32); }

__global__ void binrec_edges_kernel(BinEdgeView g, u64 lo, u64 hi, u64 *__restrict__ piece)
{
    u64 i = lo + (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i < hi; i += (u64)gridDim.x * blockDim.x) {
        const u64 src = g.src64 ? g.src64[i] : (u64)g.src32[i], e = g.ent[i], dst = ADJ_DST(e);
        const u32 f = g.edge_file ? min((u32)g.edge_file[i], g.n_files - 1) : 0u; /* writer.cpp write_binary: min(edge_file[i], n_files - 1) */
        u64 *r = piece + (i - lo) * BINREC_WORDS;
        r[0] = g.file_index ? g.file_index[src] : src + 1;
        r[1] = g.file_index ? g.file_index[dst] : dst + 1;
        r[2] = binrec_pair(ADJ_ORI(e), ADJ_OFF(e));
        r[3] = binrec_pair((u32)g.len[src], ADJ_DLEN(e));
        r[4] = (u64)f | (2ull << 16) | ((u64)(g.subs ? g.subs[i] : (u16)0) << 32); /* file, flag 2, substitutions */
    }
}

/* from the grouped and sorted rows (group_contained_rows: word / sup), with the numbers ctx_numbers derives for the text line */
__global__ void binrec_contained_kernel(CTextView g, u64 n, u32 n_files, u64 lo, u64 hi, u64 *__restrict__ piece)
{
    u64 i = lo + (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i < hi; i += (u64)gridDim.x * blockDim.x) {
        const CTextNumbers t = ctx_numbers(g, i);
        const u64 f = (u64)g.sup[i] * n_files / n; /* n < 2^31, n_files < 2^16: no overflow; writer.cpp owner_of */
        u64 *r = piece + (i - lo) * BINREC_WORDS;
        r[0] = t.a;
        r[1] = t.b;
        r[2] = binrec_pair(t.orient, t.len2);
        r[3] = binrec_pair(t.len1, t.start);
        r[4] = f; /* file, pad0 = 0, pad1 = 0 */
    }
}

#endif /* DISCO_BINREC_H_ */
