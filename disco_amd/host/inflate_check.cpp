/* inflate_check FILE — decodes a BGZF file with the decode core of the device input stage (disco_amd/csrc/disco_inflate.h) on the host,
 * one member after the other with a serial byte sink, checks every member's CRC32 and ISIZE and writes the text to stdout.
 * Exit 0, or 3 with `block N: reason` on stderr for anything it does not accept (2: usage / unreadable file).
 *
 * The members are found as the device stage finds them: by the BSIZE chain, every payload decoded inside its own bounds and to its
 * last byte. Where the chain itself does not hold (a BSIZE that is not the member's size), the file is read once more the way zlib
 * reads it — members end where their deflate streams end — and accepted, with a note on stderr, if it is sound that way: such a file
 * is valid gzip, the device stage declines it and the host stage reads it. */
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../csrc/disco_inflate.h"

namespace {
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

uint32_t crc_by_chunks(const uint8_t *p, uint32_t n)
{
    uint32_t x = 0;
    for (uint32_t lane = 0; lane < 64; lane++) x ^= infl::crc_lane(p, n, lane, 64);
    return ~x;
}

int refuse(uint64_t block, const char *why)
{
    fprintf(stderr, "block %llu: %s\n", (unsigned long long)block, why);
    return 3;
}

/* the file as a series of gzip members with BGZF-style headers, BSIZE not consulted */
int read_as_gzip(const std::vector<uint8_t> &f, std::vector<uint8_t> &text)
{
    static infl::Tables tab;
    std::vector<uint8_t> buf(INFL_MAX_ISIZE);
    uint64_t off = 0, k = 0;
    for (; off < f.size(); k++) {
        uint32_t hdr, bsize;
        const char *why = infl::bgzf_header(f.data(), f.size(), off, &hdr, &bsize);
        if (why && !hdr) return refuse(k, why);
        ByteSink sink{buf.data()};
        uint32_t used = 0, made = 0;
        const uint64_t rest = f.size() - off - hdr;
        const int e = infl::inflate_raw(f.data() + off + hdr, (uint32_t)(rest < 0xFFFFFFFFu ? rest : 0xFFFFFFFFu), INFL_MAX_ISIZE, sink, tab, 0, 1, &used, &made);
        if (e) return refuse(k, infl::reason(e));
        if (rest - used < 8) return refuse(k, "truncated trailer");
        const uint8_t *t = f.data() + off + hdr + used;
        const uint32_t crc = t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24, isize = t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
        if (isize != made) return refuse(k, infl::reason(made < isize ? infl::INFL_E_SHORT : infl::INFL_E_OUTPUT));
        if (crc != crc_by_chunks(buf.data(), made)) return refuse(k, infl::reason(infl::INFL_E_CRC));
        text.insert(text.end(), buf.begin(), buf.begin() + made);
        off += hdr + used + 8;
    }
    return k ? 0 : refuse(0, "empty file");
}
} // namespace

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: inflate_check FILE.gz\n");
        return 2;
    }
    FILE *fp = fopen(argv[1], "rb");
    if (!fp) {
        perror(argv[1]);
        return 2;
    }
    std::vector<uint8_t> f;
    uint8_t chunk[1 << 16];
    for (size_t got; (got = fread(chunk, 1, sizeof chunk, fp)) > 0;) f.insert(f.end(), chunk, chunk + got);
    fclose(fp);

    std::vector<infl::BgzfBlock> blocks;
    std::vector<uint8_t> text;
    uint64_t total = 0, bad = 0;
    int rc = 0;
    if (const char *why = infl::bgzf_walk(f.data(), f.size(), blocks, &total, &bad)) {
        uint32_t hdr, bsize;
        /* a file that begins as BGZF and whose chain breaks later: once more as plain gzip members. Anything else is refused as it stands */
        if (infl::bgzf_header(f.data(), f.size(), 0, &hdr, &bsize)) return refuse(bad, why);
        if ((rc = read_as_gzip(f, text)) != 0) return rc;
        fprintf(stderr, "note: block %llu: %s; sound as plain gzip members\n", (unsigned long long)bad, why);
    } else {
        static infl::Tables tab;
        text.resize(total);
        for (size_t k = 0; k < blocks.size(); k++) {
            const infl::BgzfBlock &b = blocks[k];
            ByteSink sink{text.data() + b.out_off};
            uint32_t used = 0, made = 0;
            int e = infl::inflate_raw(f.data() + b.in_off, b.in_len, b.isize, sink, tab, 0, 1, &used, &made);
            if (!e && made != b.isize) e = infl::INFL_E_SHORT;
            if (!e && used != b.in_len) e = infl::INFL_E_TRAIL;
            if (!e && crc_by_chunks(text.data() + b.out_off, b.isize) != b.crc) e = infl::INFL_E_CRC;
            if (e) return refuse(k, infl::reason(e));
        }
    }
    if (!text.empty() && fwrite(text.data(), 1, text.size(), stdout) != text.size()) return 2;
    return 0;
}
