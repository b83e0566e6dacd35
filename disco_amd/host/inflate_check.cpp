/* inflate_check [--window LO N] FILE — decodes a BGZF file with the decode core of the device input stage (disco_amd/csrc/disco_inflate.h)
 * on the host, one member after the other with a serial byte sink, checks every member's CRC32 and ISIZE and writes the text to stdout.
 * Exit 0, or 3 with `block N: reason` on stderr for anything it does not accept (2: usage / unreadable file).
 * --window LO N: only the bytes [LO, LO + N) of the text (what of them the text has), from the members that hold them — chosen, rebased
 * and clipped by the functions disco_inflate_bgzf_window runs; a member outside the window is not looked at, the chain is walked whole.
 *
 * The members are found as the device stage finds them: by the BSIZE chain, every payload decoded inside its own bounds and to its
 * last byte. Where the chain itself does not hold (a BSIZE that is not the member's size), the file is read once more the way zlib
 * reads it — members end where their deflate streams end — and accepted, with a note on stderr, if it is sound that way: such a file
 * is valid gzip, the device stage declines it and the host stage reads it. */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../csrc/disco_inflate.h"

namespace {
using infl::ByteSink;
using infl::crc_by_chunks;

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

/* the window [lo, lo + n) of the text to stdout: its members out of a buffer that holds their compressed bytes only, by the rebased
 * table; each one decoded and checked whole, clipped to the window as the kernel clips it */
int write_window(const std::vector<uint8_t> &f, const std::vector<infl::BgzfBlock> &blocks, uint64_t lo, uint64_t n)
{
    static infl::Tables tab;
    uint64_t first = 0, count = 0, comp_lo = 0, comp_n = 0;
    infl::bgzf_window_members(blocks, lo, n, &first, &count);
    std::vector<infl::BgzfBlock> sub;
    infl::bgzf_rebase(blocks, first, count, sub, &comp_lo, &comp_n);
    const std::vector<uint8_t> comp(f.begin() + comp_lo, f.begin() + comp_lo + comp_n); /* a copy: a read outside it is one outside an allocation */
    std::vector<uint8_t> member(INFL_MAX_ISIZE), text;
    const uint64_t hi = n > ~0ull - lo ? ~0ull : lo + n;
    for (size_t k = 0; k < sub.size(); k++) {
        const infl::BgzfBlock &b = sub[k];
        if (const int e = infl::bgzf_member_host(comp.data(), b, member.data(), tab)) return refuse(first + k, infl::reason(e));
        const uint64_t c0 = (lo > b.out_off ? lo : b.out_off) - b.out_off, end = b.out_off + b.isize, c1 = (hi < end ? hi : end) - b.out_off;
        if (c1 > c0) text.insert(text.end(), member.begin() + c0, member.begin() + c1);
    }
    if (!text.empty() && fwrite(text.data(), 1, text.size(), stdout) != text.size()) return 2;
    return 0;
}
} // namespace

int main(int argc, char **argv)
{
    const bool window = argc == 5 && strcmp(argv[1], "--window") == 0;
    char *e1 = nullptr, *e2 = nullptr;
    const uint64_t win_lo = window ? strtoull(argv[2], &e1, 10) : 0, win_n = window ? strtoull(argv[3], &e2, 10) : 0;
    if (!(argc == 2 || (window && *argv[2] && *argv[3] && !*e1 && !*e2))) {
        fprintf(stderr, "usage: inflate_check [--window LO N] FILE.gz\n");
        return 2;
    }
    const char *path = argv[argc - 1];
    FILE *fp = fopen(path, "rb");
    if (!fp) {
        perror(path);
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
    const char *why = infl::bgzf_walk(f.data(), f.size(), blocks, &total, &bad);
    if (window) {
        if (why) return refuse(bad, why);
        return write_window(f, blocks, win_lo, win_n);
    }
    if (why) {
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
            if (const int e = infl::bgzf_member_host(f.data(), b, text.data() + b.out_off, tab)) return refuse(k, infl::reason(e));
        }
    }
    if (!text.empty() && fwrite(text.data(), 1, text.size(), stdout) != text.size()) return 2;
    return 0;
}
