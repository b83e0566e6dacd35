/*
 * disco_survivor.h — the survivor list of a node: the (up to four) entries of its row that its own marking left unflagged, kept
 * aside for the emission (half[v][0 .. HALF_CAP)). Included by disco_device.h; plain C++ too, so that a host program can
 * exercise it (disco_amd/host/survivor_check.cpp).
 *
 * A list carries its own end: bit 15 of an entry — the position of ADJ_FLAG, which no entry of a list has set — marks the LAST
 * survivor. The marking sets it in the value the lane of the last survivor stores anyway, so a list costs no count: no second
 * table, no store of it per node, no clearing of it per pass, and the emission decodes the length of a neighbour's list from the
 * one 32-byte gather it needs anyway.
 *   1..4 survivors : the mark sits in slot count - 1; the slots behind it hold whatever an earlier pass left there
 *   no survivor    : slot 0 is the mark alone (no entry: the length field of an entry is a read's length, never 0)
 *   more than four : no mark in the four slots — the node is "wide" and is judged by its row
 */
#ifndef DISCO_SURVIVOR_H_
#define DISCO_SURVIVOR_H_

#if defined(__HIPCC__)
#define SURV_HD __host__ __device__ __forceinline__
#else
#define SURV_HD inline
#endif

#define SURV_CAP 4
#define SURV_WIDE (SURV_CAP + 1) /* decoded length of a list without a mark */
#define SURV_LAST (1ull << 15)
#define SURV_NONE SURV_LAST /* slot 0 of a node that has rows but no survivor */

/* the value slot r of a list of n survivors holds (entry: bit 15 clear) */
SURV_HD unsigned long long surv_encode(unsigned long long entry, unsigned r, unsigned n) { return (r + 1u == n) ? (entry | SURV_LAST) : entry; }
SURV_HD unsigned long long surv_entry(unsigned long long slot) { return slot & ~SURV_LAST; }
/* 0..4, or SURV_WIDE */
SURV_HD unsigned surv_len(unsigned long long s0, unsigned long long s1, unsigned long long s2, unsigned long long s3)
{
    if (s0 & SURV_LAST) return (s0 & 0x7FFFull) ? 1u : 0u;
    if (s1 & SURV_LAST) return 2u;
    if (s2 & SURV_LAST) return 3u;
    if (s3 & SURV_LAST) return 4u;
    return SURV_WIDE;
}
/* is `twin` (bit 15 clear, a real entry) among the survivors of the list? (false for a wide list: ask its row) */
SURV_HD bool surv_has(unsigned long long s0, unsigned long long s1, unsigned long long s2, unsigned long long s3, unsigned long long twin)
{
    const bool e0 = (s0 & SURV_LAST) != 0, e1 = e0 || (s1 & SURV_LAST), e2 = e1 || (s2 & SURV_LAST), e3 = e2 || (s3 & SURV_LAST);
    return e3 && ((surv_entry(s0) == twin) || (!e0 && surv_entry(s1) == twin) || (!e1 && surv_entry(s2) == twin) || (!e2 && surv_entry(s3) == twin));
}

#endif
