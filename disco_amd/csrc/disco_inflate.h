/*
 * disco_inflate.h — raw-deflate decoder (RFC 1951) for one BGZF member, CRC32 by chunks, and the walk over a BGZF file's member headers.
 *
 * BGZF (what bgzip / htslib write) is a series of gzip members of at most 64 KB of text each; every member carries its own compressed
 * size (the `BC` extra subfield) and its text size and CRC32 (the gzip trailer), and no back-reference crosses a member: the members
 * are independent work items with known output offsets. The input stage decodes one member per wavefront (bgzf_inflate_kernel,
 * disco_bgzf.h); the host tool disco_amd/bin/inflate_check runs the same functions serially.
 *
 * The decode core is ONE set of __host__ __device__ functions over (pointer, length) pairs. A caller is `nl` lanes that all run the
 * same code on the same values (the host: lane 0 of 1); the lanes share the tables, split the table fill among themselves and meet
 * at INFL_SYNC. Literals and (length, distance) matches go to a sink — a template parameter — AFTER the core has checked them:
 *   every read of the input is inside [in, in + n_in), every literal / match / stored run ends at or before out_cap, every distance
 *   reaches back at most to the member's first byte. A violation ends the member with an INFL_E_* code, never with an access outside.
 */
#ifndef DISCO_INFLATE_H_
#define DISCO_INFLATE_H_

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define INFL_HD __host__ __device__ inline
#else
#define INFL_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define INFL_SYNC() __syncthreads()
#else
#define INFL_SYNC() ((void)0)
#endif

namespace infl {

enum {
    INFL_OK = 0,
    INFL_E_INPUT,  /* the deflate stream runs past the member's payload                          */
    INFL_E_OUTPUT, /* more text than ISIZE                                                       */
    INFL_E_DIST,   /* a distance beyond what has been produced                                   */
    INFL_E_CODES,  /* over-subscribed or incomplete code set, bad HLIT / HDIST, bad repeat code  */
    INFL_E_BTYPE,  /* block type 3                                                               */
    INFL_E_STORED, /* stored LEN != ~NLEN                                                        */
    INFL_E_SHORT,  /* less text than ISIZE at the final block                                    */
    INFL_E_SYMBOL, /* a bit pattern no code of the set has, or a reserved symbol                 */
    INFL_E_TRAIL,  /* payload bytes left behind the final block                                  */
    INFL_E_CRC,    /* CRC32 of the text differs from the trailer's                               */
    INFL_E_COUNT
};

inline const char *reason(int e)
{
    static const char *const k[INFL_E_COUNT] = {"ok",
                                                "deflate stream runs past the payload",
                                                "more text than ISIZE",
                                                "distance beyond the start of the member",
                                                "invalid code lengths",
                                                "block type 3",
                                                "stored block length check",
                                                "less text than ISIZE",
                                                "invalid code",
                                                "payload bytes behind the final block",
                                                "CRC32 mismatch"};
    return e >= 0 && e < INFL_E_COUNT ? k[e] : "unknown error";
}

#define INFL_FAST_BITS 10
#define INFL_FAST_SIZE (1 << INFL_FAST_BITS)

/* decode tables of one deflate block: a first-level table over INFL_FAST_BITS bits (entry = symbol << 4 | code length, 0 = not there)
 * and the canonical form (count per length + symbols in code order) for longer codes. 5.2 KB: LDS on the device */
struct Tables {
    uint16_t fast_ll[INFL_FAST_SIZE], fast_d[INFL_FAST_SIZE];
    uint16_t sym_ll[288], sym_d[32];
    uint16_t cnt_ll[16], cnt_d[16];
    uint16_t offs[16];
    uint8_t lens[320]; /* code lengths as the dynamic header gives them: literal/length codes, then distance codes */
};

struct Bits {
    const uint8_t *in;
    uint32_t n, pos; /* pos: next byte to load */
    uint64_t hold;   /* bits [0, nbits) are the stream's next bits; bits above are zero or a copy of what comes next */
    uint32_t nbits;
    uint64_t ahead;  /* the eight bytes at pos, loaded when pos was set (where eight are left): the next refill does not wait for memory */
};

INFL_HD void look_ahead(Bits &b)
{
    if (b.n - b.pos >= 8) __builtin_memcpy(&b.ahead, b.in + b.pos, 8);
}

/* at least 32 bits afterwards unless the input ends: a code and its extra bits are 28 at most, a stored block's lengths 32. The load
 * it needs was issued by the refill before it — a load per symbol, waited for on the spot, was three quarters of the kernel's time */
INFL_HD void refill(Bits &b)
{
    if (b.nbits >= 32) return;
    if (b.n - b.pos >= 8) {
        b.hold |= b.ahead << b.nbits;
        const uint32_t k = (63 - b.nbits) >> 3;
        b.pos += k;
        b.nbits += 8 * k;
        look_ahead(b);
    } else
        while (b.nbits <= 56 && b.pos < b.n) {
            b.hold |= (uint64_t)b.in[b.pos++] << b.nbits;
            b.nbits += 8;
        }
}

/* n <= 32 bits, least significant first; past the end of the input: 0 and *err = INFL_E_INPUT */
INFL_HD uint32_t take(Bits &b, uint32_t n, int *err)
{
    refill(b);
    if (b.nbits < n) {
        *err = INFL_E_INPUT;
        return 0;
    }
    const uint32_t v = (uint32_t)(b.hold & ((1ull << n) - 1));
    b.hold >>= n;
    b.nbits -= n;
    return v;
}

INFL_HD uint32_t bit_reverse(uint32_t v, uint32_t n)
{
    uint32_t r = 0;
    for (uint32_t i = 0; i < n; i++) r |= ((v >> i) & 1u) << (n - 1 - i);
    return r;
}

/* the tables of one code set from its n code lengths. zlib's rule: an over-subscribed set is an error; an incomplete one too, unless
 * `single_ok` (distance codes) and the set has no code at all or one code of one bit — a pattern outside the set is then an error
 * where it is met. The serial parts run on every lane alike, the fill of the first-level table is dealt out by lane. */
INFL_HD int build(uint16_t *fast, uint16_t *cnt, uint16_t *sym, uint16_t *offs, const uint8_t *lens, uint32_t n, bool single_ok, uint32_t lane, uint32_t nl)
{
    INFL_SYNC(); /* whoever still reads the tables being replaced */
    for (uint32_t i = lane; i < INFL_FAST_SIZE; i += nl) fast[i] = 0;
    for (uint32_t l = 0; l < 16; l++) cnt[l] = 0;
    for (uint32_t s = 0; s < n; s++) cnt[lens[s]]++;
    int left = 1;
    for (uint32_t l = 1; l < 16; l++) {
        left <<= 1;
        left -= (int)cnt[l];
        if (left < 0) return INFL_E_CODES;
    }
    const uint32_t total = n - cnt[0];
    if (left > 0 && !(single_ok && (total == 0 || (total == 1 && cnt[1] == 1)))) return INFL_E_CODES;
    offs[1] = 0;
    for (uint32_t l = 1; l < 15; l++) offs[l + 1] = (uint16_t)(offs[l] + cnt[l]);
    for (uint32_t s = 0; s < n; s++)
        if (lens[s]) sym[offs[lens[s]]++] = (uint16_t)s; /* offs[l] ends as the index behind the last symbol of length l */
    INFL_SYNC();
    for (uint32_t i = lane; i < total; i += nl) {
        const uint32_t s = sym[i], l = lens[s];
        if (l > INFL_FAST_BITS) continue;
        uint32_t first = 0; /* canonical code of the first symbol of length l */
        for (uint32_t k = 1; k < l; k++) first = (first + cnt[k]) << 1;
        const uint32_t code = first + (i - (uint32_t)(offs[l] - cnt[l]));
        for (uint32_t j = bit_reverse(code, l); j < INFL_FAST_SIZE; j += 1u << l) fast[j] = (uint16_t)(s << 4 | l);
    }
    INFL_SYNC();
    return INFL_OK;
}

INFL_HD uint32_t decode_sym(Bits &b, const uint16_t *fast, const uint16_t *cnt, const uint16_t *sym, int *err)
{
    refill(b);
    const uint32_t e = fast[b.hold & (INFL_FAST_SIZE - 1)];
    if (e) {
        const uint32_t l = e & 15;
        if (l > b.nbits) {
            *err = INFL_E_INPUT;
            return 0;
        }
        b.hold >>= l;
        b.nbits -= l;
        return e >> 4;
    }
    /* a code longer than the first-level table, or no code at all: walk the canonical code bit by bit */
    int code = 0, first = 0, index = 0;
    uint64_t h = b.hold;
    for (uint32_t l = 1; l <= 15; l++) {
        code |= (int)(h & 1);
        h >>= 1;
        const int count = cnt[l];
        if (code - count < first) {
            if (l > b.nbits) {
                *err = INFL_E_INPUT;
                return 0;
            }
            b.hold >>= l;
            b.nbits -= l;
            return sym[index + (code - first)];
        }
        index += count;
        first += count;
        first <<= 1;
        code <<= 1;
    }
    *err = b.nbits < 15 ? INFL_E_INPUT : INFL_E_SYMBOL;
    return 0;
}

/* Decodes one raw deflate stream in[0, n_in) up to its final block. The sink receives
 *     lit(byte)   match(length, distance)   raw(pointer, count)   (a stored block's bytes, inside the input)
 * in output order, each one checked: the text never exceeds out_cap and no distance reaches in front of it. *consumed = input bytes
 * used (the final block's last byte counts whole), *produced = text bytes. Returns INFL_OK or the first error. */
template <class Sink>
INFL_HD int inflate_raw(const uint8_t *in, uint32_t n_in, uint32_t out_cap, Sink &sink, Tables &t, uint32_t lane, uint32_t nl, uint32_t *consumed, uint32_t *produced)
{
    Bits b = {in, n_in, 0, 0, 0, 0};
    look_ahead(b);
    uint32_t out = 0;
    int err = INFL_OK;
    *consumed = 0;
    *produced = 0;
    for (;;) {
        const uint32_t bfinal = take(b, 1, &err), btype = take(b, 2, &err);
        if (err) return err;
        if (btype == 3) return INFL_E_BTYPE;
        if (btype == 0) {
            take(b, b.nbits & 7, &err); /* to the byte boundary */
            const uint32_t v = take(b, 32, &err);
            if (err) return err;
            const uint32_t len = v & 0xFFFFu;
            if (len != ((~v >> 16) & 0xFFFFu)) return INFL_E_STORED;
            b.pos -= b.nbits >> 3; /* whole bytes in the bit buffer go back */
            b.hold = 0;
            b.nbits = 0;
            if (len > b.n - b.pos) return INFL_E_INPUT;
            if (len > out_cap - out) return INFL_E_OUTPUT;
            if (len) sink.raw(in + b.pos, len);
            b.pos += len;
            look_ahead(b);
            out += len;
        } else {
            if (btype == 1) {
                INFL_SYNC();
                for (uint32_t s = 0; s < 288; s++) t.lens[s] = (uint8_t)(s < 144 ? 8 : (s < 256 ? 9 : (s < 280 ? 7 : 8)));
                for (uint32_t s = 0; s < 32; s++) t.lens[288 + s] = 5;
                if ((err = build(t.fast_ll, t.cnt_ll, t.sym_ll, t.offs, t.lens, 288, false, lane, nl)) != INFL_OK) return err;
                if ((err = build(t.fast_d, t.cnt_d, t.sym_d, t.offs, t.lens + 288, 32, false, lane, nl)) != INFL_OK) return err;
            } else {
                const uint32_t hlit = take(b, 5, &err) + 257, hdist = take(b, 5, &err) + 1, hclen = take(b, 4, &err) + 4;
                if (err) return err;
                if (hlit > 286 || hdist > 30) return INFL_E_CODES;
                INFL_SYNC();
                for (uint32_t i = 0; i < 19; i++) t.lens[i] = 0;
                for (uint32_t i = 0; i < hclen; i++) {
                    /* 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, five bits each */
                    const uint32_t o = i < 12 ? (uint32_t)((0x22caa324e804a30ull >> (5 * i)) & 31) : (uint32_t)((0x3c2e1346cull >> (5 * (i - 12))) & 31);
                    t.lens[o] = (uint8_t)take(b, 3, &err);
                }
                if (err) return err;
                if ((err = build(t.fast_d, t.cnt_d, t.sym_d, t.offs, t.lens, 19, false, lane, nl)) != INFL_OK) return err;
                const uint32_t n_len = hlit + hdist;
                for (uint32_t i = 0; i < n_len;) {
                    const uint32_t s = decode_sym(b, t.fast_d, t.cnt_d, t.sym_d, &err);
                    if (err) return err;
                    if (s < 16) {
                        t.lens[i++] = (uint8_t)s;
                        continue;
                    }
                    uint32_t v = 0, rep;
                    if (s == 16) {
                        if (i == 0) return INFL_E_CODES;
                        v = t.lens[i - 1];
                        rep = 3 + take(b, 2, &err);
                    } else if (s == 17)
                        rep = 3 + take(b, 3, &err);
                    else
                        rep = 11 + take(b, 7, &err);
                    if (err) return err;
                    if (rep > n_len - i) return INFL_E_CODES;
                    while (rep--) t.lens[i++] = (uint8_t)v;
                }
                if (t.lens[256] == 0) return INFL_E_CODES; /* no end-of-block code */
                if ((err = build(t.fast_ll, t.cnt_ll, t.sym_ll, t.offs, t.lens, hlit, false, lane, nl)) != INFL_OK) return err;
                if ((err = build(t.fast_d, t.cnt_d, t.sym_d, t.offs, t.lens + hlit, hdist, true, lane, nl)) != INFL_OK) return err;
            }
            for (;;) {
                const uint32_t s = decode_sym(b, t.fast_ll, t.cnt_ll, t.sym_ll, &err);
                if (err) return err;
                if (s < 256) {
                    if (out >= out_cap) return INFL_E_OUTPUT;
                    sink.lit((uint8_t)s);
                    out++;
                    continue;
                }
                if (s == 256) break;
                if (s > 285) return INFL_E_SYMBOL;
                uint32_t len, dist;
                const uint32_t li = s - 257;
                if (li < 8)
                    len = 3 + li;
                else if (li == 28)
                    len = 258;
                else {
                    const uint32_t e = (li >> 2) - 1;
                    len = 3 + ((4 + (li & 3)) << e) + take(b, e, &err);
                }
                const uint32_t d = decode_sym(b, t.fast_d, t.cnt_d, t.sym_d, &err);
                if (err) return err;
                if (d >= 30) return INFL_E_SYMBOL;
                if (d < 4)
                    dist = 1 + d;
                else {
                    const uint32_t e = (d >> 1) - 1;
                    dist = 1 + ((2 + (d & 1)) << e) + take(b, e, &err);
                }
                if (err) return err;
                if (dist > out) return INFL_E_DIST;
                if (len > out_cap - out) return INFL_E_OUTPUT;
                sink.match(len, dist);
                out += len;
            }
        }
        if (bfinal) break;
    }
    *consumed = b.pos - (b.nbits >> 3);
    *produced = out;
    return INFL_OK;
}

/* ---- CRC32 (the gzip polynomial, reflected) by chunks ------------------------------------------------------------------------- */
#define INFL_CRC_POLY 0xEDB88320u

/* the CRC register after the bytes p[0, n), from `state` (no pre- / post-inversion) */
INFL_HD uint32_t crc_bytes(uint32_t state, const uint8_t *p, uint32_t n)
{
    for (uint32_t i = 0; i < n; i++) {
        state ^= p[i];
        for (int k = 0; k < 8; k++) state = (state >> 1) ^ (INFL_CRC_POLY & (0u - (state & 1u)));
    }
    return state;
}

/* a * b mod P over GF(2), reflected: bit 31 is x^0 */
INFL_HD uint32_t gf_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 0; i < 32; i++) {
        p ^= b & (0u - ((a >> (31 - i)) & 1u));
        b = (b >> 1) ^ (INFL_CRC_POLY & (0u - (b & 1u)));
    }
    return p;
}

/* the register `state` after n more zero bytes = state * x^(8n) mod P */
INFL_HD uint32_t crc_shift(uint32_t state, uint32_t n)
{
    uint32_t r = 0x80000000u, sq = 0x00800000u; /* x^0, x^8 */
    for (; n; n >>= 1) {
        if (n & 1) r = gf_mul(r, sq);
        sq = gf_mul(sq, sq);
    }
    return gf_mul(r, state);
}

/* lane's share of the CRC32 of p[0, n): the register over its chunk (the first chunk starts from all ones), moved behind the last
 * byte. The XOR over all nl lanes, inverted, is the CRC32. */
INFL_HD uint32_t crc_lane(const uint8_t *p, uint32_t n, uint32_t lane, uint32_t nl)
{
    const uint32_t chunk = (n + nl - 1) / nl;
    const uint32_t lo = lane * chunk < n ? lane * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
    const uint32_t st = crc_bytes(lane == 0 ? 0xFFFFFFFFu : 0u, p + lo, hi - lo);
    return st ? crc_shift(st, n - hi) : 0u;
}

/* ---- the member chain of a BGZF buffer (host) ---------------------------------------------------------------------------------- */
#define INFL_MAX_ISIZE 65536u

struct BgzfBlock {
    uint64_t in_off;  /* the member's deflate payload: bytes [in_off, in_off + in_len) of the buffer */
    uint64_t out_off; /* its text: bytes [out_off, out_off + isize) of the output               */
    uint32_t in_len, isize, crc, pad_;
};

/* one member header at d + off: 1f 8b 08, FEXTRA set (FTEXT may be), a `BC` subfield of length 2 among the extra subfields.
 * *hdr = bytes in front of the payload, *bsize = the member's size by its BC subfield (0: none). Returns null or what is wrong. */
inline const char *bgzf_header(const uint8_t *d, uint64_t n, uint64_t off, uint32_t *hdr, uint32_t *bsize)
{
    *hdr = 0;
    *bsize = 0;
    if (n - off < 12) return "truncated header";
    const uint8_t *h = d + off;
    if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8) return "not a gzip member";
    if (!(h[3] & 4) || (h[3] & ~5)) return "not a BGZF member (flags)";
    const uint32_t xlen = h[10] | (uint32_t)h[11] << 8;
    if (n - off - 12 < xlen) return "truncated header";
    for (uint32_t x = 0; x + 4 <= xlen;) {
        const uint8_t *s = h + 12 + x;
        const uint32_t slen = s[2] | (uint32_t)s[3] << 8;
        if (slen > xlen - x - 4) return "extra subfield beyond XLEN";
        if (s[0] == 'B' && s[1] == 'C' && slen == 2 && !*bsize) *bsize = (s[4] | (uint32_t)s[5] << 8) + 1;
        x += 4 + slen;
    }
    *hdr = 12 + xlen;
    return *bsize ? nullptr : "not a BGZF member (no BC subfield)";
}

/* walks the BSIZE chain of d[0, n): every member must be BGZF, the chain must end exactly at n, ISIZE <= 64 KB. Empty members are
 * legal anywhere, the empty end-of-file member may be missing. Returns null and the blocks (Vec: any push_back container of
 * BgzfBlock), or what is wrong with member *bad. */
template <class Vec>
inline const char *bgzf_walk(const uint8_t *d, uint64_t n, Vec &blocks, uint64_t *total, uint64_t *bad)
{
    uint64_t off = 0, out = 0, k = 0;
    *total = 0;
    for (; off < n; k++) {
        uint32_t hdr, bsize;
        *bad = k;
        if (const char *why = bgzf_header(d, n, off, &hdr, &bsize)) return why;
        if (bsize < hdr + 8 + 1) return "BSIZE smaller than header and trailer";
        if (bsize > n - off) return "BSIZE beyond the end of the file";
        const uint8_t *t = d + off + bsize - 8;
        BgzfBlock b;
        b.in_off = off + hdr;
        b.in_len = bsize - hdr - 8;
        b.crc = t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
        b.isize = t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
        b.out_off = out;
        b.pad_ = 0;
        if (b.isize > INFL_MAX_ISIZE) return "ISIZE beyond 64 KB";
        blocks.push_back(b);
        out += b.isize;
        off += bsize;
    }
    *bad = k;
    *total = out;
    return k ? nullptr : "empty file";
}

/* the members that hold the window [lo, lo + n) of the text: blocks [*first, *first + *count), ONE range of the chain (out_off never
 * decreases along it). Its first and its last member hold a byte of the window; empty members between them belong to it, empty members
 * on its edges do not. count 0: the window is empty or lies behind the text. Blocks: anything with size() and [] of BgzfBlock. */
template <class Blocks>
inline void bgzf_window_members(const Blocks &blocks, uint64_t lo, uint64_t n, uint64_t *first, uint64_t *count)
{
    const uint64_t nb = blocks.size(), hi = n > ~0ull - lo ? ~0ull : lo + n;
    uint64_t a = 0, b = nb;
    while (a < b) { /* the first member that ends behind lo */
        const uint64_t m = a + (b - a) / 2;
        if (blocks[m].out_off + blocks[m].isize > lo) b = m;
        else a = m + 1;
    }
    *first = a;
    for (b = nb; a < b;) { /* the first member that begins at or behind hi */
        const uint64_t m = a + (b - a) / 2;
        if (blocks[m].out_off >= hi) b = m;
        else a = m + 1;
    }
    while (a > *first && blocks[a - 1].isize == 0) a--;
    *count = a > *first && n ? a - *first : 0;
}

/* the table of a launch (or of the host tool's loop) over the members [first, first + count): in_off counts from the first one's
 * payload, whose offset in the file is *comp_lo; the members' compressed bytes, headers and trailers between them included, are
 * [*comp_lo, *comp_lo + *comp_n) of the file. out_off stays what it is: the member's place in the file's text */
template <class Blocks, class Vec>
inline void bgzf_rebase(const Blocks &blocks, uint64_t first, uint64_t count, Vec &out, uint64_t *comp_lo, uint64_t *comp_n)
{
    out.clear();
    *comp_lo = count ? blocks[first].in_off : 0;
    *comp_n = count ? blocks[first + count - 1].in_off + blocks[first + count - 1].in_len - *comp_lo : 0;
    for (uint64_t k = first; k < first + count; k++) {
        BgzfBlock b = blocks[k];
        b.in_off -= *comp_lo;
        out.push_back(b);
    }
}

/* ---- one member on the host: a serial byte sink, the CRC32 by the lanes' chunks (inflate_check; the first and the last byte of a file
 * for the ranks of disco_dist_ingest_fasta) ------------------------------------------------------------------------------------------ */
struct ByteSink {
    uint8_t *out;
    uint32_t p = 0;
    void lit(uint8_t c) { out[p++] = c; }
    void match(uint32_t len, uint32_t dist)
    {
        for (uint32_t i = 0; i < len; i++) out[p + i] = out[p - dist + (i < dist ? i : i % dist)]; /* the lanes' formula */
        p += len;
    }
    void raw(const uint8_t *s, uint32_t n)
    {
        memcpy(out + p, s, n);
        p += n;
    }
};

inline uint32_t crc_by_chunks(const uint8_t *p, uint32_t n)
{
    uint32_t x = 0;
    for (uint32_t lane = 0; lane < 64; lane++) x ^= crc_lane(p, n, lane, 64);
    return ~x;
}

/* member b, whose payload lies at comp + b.in_off, decoded whole into out[0, b.isize) and checked as the kernel checks it: INFL_* */
inline int bgzf_member_host(const uint8_t *comp, const BgzfBlock &b, uint8_t *out, Tables &tab)
{
    ByteSink sink{out};
    uint32_t used = 0, made = 0;
    int e = inflate_raw(comp + b.in_off, b.in_len, b.isize, sink, tab, 0, 1, &used, &made);
    if (!e && made != b.isize) e = INFL_E_SHORT;
    if (!e && used != b.in_len) e = INFL_E_TRAIL;
    if (!e && crc_by_chunks(out, b.isize) != b.crc) e = INFL_E_CRC;
    return e;
}

} // namespace infl
#endif
