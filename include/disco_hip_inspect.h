/*
 * disco_hip_inspect.h — entry points of libdisco_hip.so that let a test LOOK at intermediate state no result depends on. Same library,
 * same C rules as include/disco_hip.h; not part of the boundary a BuildGraph host binds, and not among the bench / test entry points of
 * include/disco_hip_test.h, whose set is pinned: the Python mirror binds these on first use (disco_amd/buildgraph.py, INSPECT_ABI).
 */
#ifndef DISCO_HIP_INSPECT_H_
#define DISCO_HIP_INSPECT_H_

#include "disco_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the processing order the last disco_build_index made (results do not depend on it, so only a look at it shows a grouping that stopped
 * grouping): order_words[0 .. *n) = read id | length << 32 in the order probe / verify / selection / marking walk, keys[read] = the reads'
 * grouping keys; reads whose (key * 0x9E3779B1) >> (32 - *order_bits) agree lie back to back. cap: room in both arrays, in entries (too
 * little: *n and *order_bits are set, DISCO_E_ARG). DISCO_E_STATE when the last index build made no order (fewer reads than the grouping
 * takes, two classes of rows, a caller's order, DISCO_NO_ORDER). Tests only. */
int disco_fetch_order(disco_ctx *ctx, uint64_t *order_words, uint32_t *keys, uint64_t cap, uint64_t *n, int *order_bits);

/* the sub-key of the binned grouping (results do not depend on it): inside an order bucket the reads lie in the order of
 * sub = min((start_rel * floor(2^(b + 16) / P)) >> 16, 2^b - 1), b = *in_use, not decreasing — start_rel = the position of the read's
 * minimizer occurrence (among its m-mers the one with the smallest order hash >> 9, the leftmost of equal ones) if the m-mer is the
 * canonical one as it stands in the read, the read's m-mer positions - 1 - that position otherwise; P = the m-mer positions of the table's
 * longest read. *in_use (may be null): the bits the last disco_build_index gave it — what bucket, length and
 * read id leave of an item's 64, at most 3; 0: no binned grouping, no minimizer runs, or no bit left. bits >= 0: later index builds use at
 * most that many (0: the item as it was before the sub-key); bits < 0: only the look. Tests only. */
int disco_set_order_sub_bits(disco_ctx *ctx, int bits, int *in_use);

/* how the last disco_transitive_reduce laid its survivors out (results do not depend on it): *dense = 1 if the emission wrote its edges
 * back to back (no unused chunk tails: *out_used, the slots it wrote, is then the number of edges), list_len[v] = the decoded length of
 * node v's self-delimiting survivor list (disco_amd/csrc/disco_survivor.h): 0..4, 5 = wide (more than four survivors, judged by its row),
 * 0xFF = the node has no row, so the marking wrote no list for it. list_len may be null (the other three only); cap: its room, in nodes
 * (*n is set; too little: DISCO_E_ARG). DISCO_E_STATE for the lengths when the last marking kept counts instead (flows that need every
 * row's flags, or a communicator). Tests only. */
int disco_fetch_survivor_layout(disco_ctx *ctx, uint8_t *list_len, uint64_t cap, uint64_t *n, int *dense, uint64_t *out_used);

/* records per piece of disco_fetch_*_records / disco_write_*_records (results do not depend on it): 0 = the default, as many as a half of
 * the pinned ring holds (3 355 443) — with which a small test would never cross a piece boundary; larger values are cut to the default.
 * Tests only. */
int disco_set_record_piece(disco_ctx *ctx, uint64_t records);

#ifdef __cplusplus
}
#endif
#endif /* DISCO_HIP_INSPECT_H_ */
