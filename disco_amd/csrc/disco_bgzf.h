/*
 * disco_bgzf.h — bgzf_inflate_kernel: the members of a BGZF file, one wavefront each, from the compressed bytes in HBM to the text
 * the record kernels of disco_ingest.h read. The decoder is disco_inflate.h (the host tool inflate_check runs the same functions).
 *
 * Form: a block is one wavefront. The decode state is the same in all 64 lanes (every lane walks the bit stream; nothing is
 * broadcast); the code tables (5.2 KB) and the member's whole text window (64 KB: ISIZE never exceeds it, back-references never
 * leave the member) are in LDS — 70 KB a block, two blocks a CU. Literals collect in a register, eight to a store instruction;
 * a match is copied by the lanes side by side, out[p + i] = out[p - d + i % d] (a distance below the length repeats its period).
 * The CRC32 is taken over the window — a chunk per lane, the registers moved to the end by multiplying with x^(8 n) mod P and
 * XORed over the wave — and only a member that is sound is written out, 16 bytes a lane where source and destination allow it (the
 * window is laid into LDS at the destination's misalignment, so they always do between the first and the last few bytes).
 * A launch writes a WINDOW of the file's text: a member is decoded and checked whole, and of its bytes those inside the window are
 * stored, at text + (out_off + i - win_lo) — a whole file is the window [0, its text); a rank's piece of it is decoded from the
 * members that overlap the piece, the first and the last of them clipped.
 * Nothing the wave has stored is read back through global memory.
 */
#ifndef DISCO_BGZF_H_
#define DISCO_BGZF_H_

#include "disco_device.h"
#include "disco_inflate.h"

struct BgzfArgs {
    const u8 *comp;              /* the compressed bytes of the launched members: in_off counts from here */
    const infl::BgzfBlock *blk;  /* the launched members; out_off is a member's place in the FILE's text  */
    u32 n_blk;
    u8 *text;                    /* the window's first byte: text[0, win_n) is all a launch may write     */
    u64 win_lo, win_n;           /* the window of the file's text (a whole file: 0 and its text's size)   */
    u32 *status;                 /* [n_blk] INFL_* of every member, then one word: members with an error */
};

struct WaveSink {
    u8 *w; /* LDS: w[0] is the member's first text byte */
    u32 p, lane;
    u64 acc; /* literals not yet stored, first one lowest */
    u32 nacc;
    __device__ void flush()
    {
        if (nacc) {
            if (lane < nacc) w[p + lane] = (u8)(acc >> (8 * lane));
            p += nacc;
            acc = 0;
            nacc = 0;
        }
    }
    __device__ void lit(u8 c)
    {
        acc |= (u64)c << (8 * nacc);
        if (++nacc == 8) flush();
    }
    __device__ void match(u32 len, u32 dist)
    {
        flush();
        __syncthreads(); /* one wave: orders the LDS stores in front of the loads below */
        for (u32 i = lane; i < len; i += 64) w[p + i] = w[p - dist + (i < dist ? i : i % dist)];
        p += len;
    }
    __device__ void raw(const u8 *s, u32 n)
    {
        flush();
        for (u32 i = lane; i < n; i += 64) w[p + i] = s[i];
        p += n;
    }
};

__global__ void __launch_bounds__(64) bgzf_inflate_kernel(BgzfArgs a)
{
    __shared__ __attribute__((aligned(16))) u8 win[INFL_MAX_ISIZE + 16];
    __shared__ infl::Tables tab;
    const u32 m = blockIdx.x, lane = threadIdx.x;
    if (m >= a.n_blk) return;
    const infl::BgzfBlock b = a.blk[m];
    /* where the member's first byte would lie, as a number: in front of `text` where the window cuts the member's front, and never dereferenced there */
    const uintptr_t dst = (uintptr_t)a.text + (uintptr_t)(b.out_off - a.win_lo);
    const u32 mis = (u32)(dst & 15u);
    /* the member's bytes [c0, c1) lie in the window: dst + i is inside text[0, win_n) exactly for them (known in front of the decode, so
     * that the window does not stay in registers through it) */
    const u64 m_lo = b.out_off, m_hi = m_lo + b.isize, w_hi = a.win_lo + a.win_n;
    const u32 c0 = (u32)(min(max(m_lo, a.win_lo), m_hi) - m_lo), c1 = (u32)(max(min(m_hi, w_hi), m_lo + c0) - m_lo);
    WaveSink sink = {win + mis, 0, lane, 0, 0};
    u32 used = 0, made = 0;
    int err = infl::inflate_raw(a.comp + b.in_off, b.in_len, b.isize, sink, tab, lane, 64, &used, &made);
    sink.flush();
    __syncthreads();
    if (!err && made != b.isize) err = infl::INFL_E_SHORT;
    if (!err && used != b.in_len) err = infl::INFL_E_TRAIL;
    if (!err) {
        u32 x = infl::crc_lane(sink.w, b.isize, lane, 64);
        for (int o = 32; o; o >>= 1) x ^= (u32)__shfl_xor((int)x, o);
        if (~x != b.crc) err = infl::INFL_E_CRC;
    }
    if (!err) {
        const u8 *w = sink.w;
        const u32 n = c1 - c0, head = min(n, (16u - ((mis + c0) & 15u)) & 15u), body = (n - head) / 16;
        if (lane < head) *(u8 *)(dst + c0 + lane) = w[c0 + lane];
        for (u32 i = lane; i < body; i += 64) *(uint4 *)(dst + c0 + head + 16 * i) = *(const uint4 *)(w + c0 + head + 16 * i);
        for (u32 i = c0 + head + 16 * body + lane; i < c1; i += 64) *(u8 *)(dst + i) = w[i];
    }
    if (lane == 0) {
        a.status[m] = (u32)err;
        if (err) atomicAdd(a.status + a.n_blk, 1u);
    }
}

#endif
