/*
 * gfa_check — the line and item functions behind <prefix>.gfa (disco_amd/csrc/disco_gfa.h) on the host: the same header the kernels
 * include, built as plain C++, one "lane" after the other. tests/test_gfa_host.py writes a case and compares the text.
 *   gfa_check <case file>        -> the file's text on stdout
 * The case file, tokens separated by white space:
 *   n_reads has_file_index layout stride no_seq max_substitutions
 *       layout 0: rows of one stride of `stride` words; 1: two classes — 8-word rows for everybody, rows of `stride` words for the reads
 *       of more than 256 bases
 *   per read: its bases (ACGT) [its file index, if has_file_index]
 *   n_edges then per edge: src dst orient offset substitutions            (read ids; src's length - offset = the overlap)
 *   n_rows  then per contained row: container contained orient start      (read ids; start = len1 - overlapLen)
 * Measure -> scan -> write as disco_write_gfa does, the S lines item by item in the kernels' two passes, so that the byte counts are
 * checked against what is written, and every byte of the text against having been written at all.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../csrc/disco_gfa.h"

static bool bad(const char *what)
{
    fprintf(stderr, "gfa_check: %s\n", what);
    return false;
}

static bool run(FILE *f)
{
    unsigned long long v[6];
    auto get = [&](unsigned long long *out, int m) {
        for (int i = 0; i < m; i++)
            if (fscanf(f, "%llu", &out[i]) != 1) return false;
        return true;
    };
    if (!get(v, 6)) return bad("header");
    const uint64_t n = v[0];
    const bool has_fi = v[1] != 0, classes = v[2] != 0, no_seq = v[4] != 0, has_nm = v[5] != 0;
    const uint32_t stride = (uint32_t)v[3];
    if (stride == 0 || (classes && stride <= GFA_HEAD_WORDS)) return bad("stride");
    std::vector<uint16_t> len(n);
    std::vector<uint64_t> fi(has_fi ? n : 0);
    std::vector<uint32_t> ovf(n), long_ids;
    std::vector<std::string> seq(n);
    std::vector<char> word(40000);
    for (uint64_t i = 0; i < n; i++) {
        if (fscanf(f, "%39999s", word.data()) != 1) return bad("a read");
        seq[i] = word.data();
        if (seq[i].empty() || seq[i].size() > 32767 || seq[i].size() > 32u * stride) return bad("a read's length");
        len[i] = (uint16_t)seq[i].size();
        if (has_fi) {
            if (!get(v, 1)) return bad("a file index");
            fi[i] = v[0];
        }
        ovf[i] = (uint32_t)long_ids.size();
        if (classes && len[i] > GFA_SHORT_MAX) long_ids.push_back((uint32_t)i);
    }
    /* the table: 2 bits a base, MSB first, A0 C1 G2 T3, unused bits zero */
    const uint32_t S = classes ? GFA_HEAD_WORDS : stride;
    std::vector<uint64_t> rows((n + long_ids.size()) * S + 1, 0), full(long_ids.size() * (size_t)stride + 1, 0);
    for (uint64_t i = 0; i < n; i++) {
        const bool is_long = classes && len[i] > GFA_SHORT_MAX;
        for (uint32_t b = 0; b < len[i]; b++) {
            uint64_t code;
            switch (seq[i][b]) {
            case 'A': code = 0; break;
            case 'C': code = 1; break;
            case 'G': code = 2; break;
            case 'T': code = 3; break;
            default: return bad("a base that is not ACGT");
            }
            const uint64_t bit = code << (62 - 2 * (b & 31u));
            if (b < 32u * S) rows[i * S + (b >> 5)] |= bit; /* (a long read's 64-byte row holds its head) */
            if (is_long) full[(size_t)ovf[i] * stride + (b >> 5)] |= bit;
        }
    }
    GfaReads g;
    g.rows = rows.data();
    g.full = classes ? full.data() : nullptr;
    g.ovf = classes ? ovf.data() : nullptr;
    g.long_ids = classes ? long_ids.data() : nullptr;
    g.len = len.data();
    g.file_index = has_fi ? fi.data() : nullptr;
    g.n = n;
    g.S = S;
    g.SL = classes ? stride : 0;

    if (!get(v, 1)) return bad("edges");
    std::vector<GfaL> edges(v[0]);
    for (auto &e : edges) {
        if (!get(v, 5)) return bad("edge");
        if (v[0] >= n || v[1] >= n || v[2] > 3 || v[3] >= len[v[0]]) return bad("an edge names no read, orientation or offset");
        e.a = gfa_name(g, v[0]);
        e.b = gfa_name(g, v[1]);
        e.orient = (uint32_t)v[2];
        e.ovl = len[v[0]] - (uint32_t)v[3];
        e.nm = (uint32_t)v[4];
        e.has_nm = has_nm;
    }
    if (!get(v, 1)) return bad("contained rows");
    std::vector<GfaC> crows(v[0]);
    for (auto &r : crows) {
        if (!get(v, 4)) return bad("contained row");
        if (v[0] >= n || v[1] >= n || v[2] > 3 || v[3] + len[v[1]] > len[v[0]]) return bad("a contained row names no read, orientation or place");
        r = gfa_c_of(gfa_name(g, v[0]), gfa_name(g, v[1]), (uint32_t)v[2], len[v[0]], len[v[1]], (uint32_t)v[3]);
    }

    /* measure, scan */
    const std::string header = GFA_HEADER;
    std::vector<uint64_t> splace(n + 1, header.size());
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t b = gfa_s_bytes(gfa_name(g, i), len[i], no_seq);
        if (b > GFA_MAX_LINE) return bad("a line longer than GFA_MAX_LINE");
        splace[i + 1] = splace[i] + b;
    }
    std::vector<uint64_t> lplace(edges.size() + 1, splace[n]);
    for (size_t i = 0; i < edges.size(); i++) lplace[i + 1] = lplace[i] + gfa_l_bytes(edges[i]);
    std::vector<uint64_t> cplace(crows.size() + 1, lplace[edges.size()]);
    for (size_t i = 0; i < crows.size(); i++) cplace[i + 1] = cplace[i] + gfa_c_bytes(crows[i]);
    std::vector<char> text(cplace[crows.size()], 0);
    header.copy(text.data(), header.size());

    /* write: the S lines as gfa_s_write_kernel and gfa_s_write_long_kernel deal the words out */
    const uint32_t W = no_seq ? 1u : S;
    for (uint64_t i = 0; i < n; i++)
        for (uint32_t w = 0; w < W; w++) {
            if (w >= gfa_s_items(len[i], no_seq)) continue;
            gfa_s_put(text.data() + splace[i], gfa_name(g, i), len[i], w, no_seq ? 0 : gfa_word(g, i, w), no_seq);
        }
    if (classes && !no_seq)
        for (size_t j = 0; j < long_ids.size(); j++)
            for (uint32_t w = GFA_HEAD_WORDS; w < stride; w++) {
                const uint64_t i = long_ids[j];
                if (w >= gfa_s_items(len[i], false)) continue;
                gfa_s_put(text.data() + splace[i], gfa_name(g, i), len[i], w, full[j * (size_t)stride + w], false);
            }
    for (size_t i = 0; i < edges.size(); i++)
        if (gfa_l_put(text.data() + lplace[i], edges[i]) != text.data() + lplace[i + 1]) return bad("an L line of another number of bytes than measured");
    for (size_t i = 0; i < crows.size(); i++)
        if (gfa_c_put(text.data() + cplace[i], crows[i]) != text.data() + cplace[i + 1]) return bad("a C line of another number of bytes than measured");
    for (uint64_t i = 0; i < n; i++)
        if (text[splace[i + 1] - 1] != '\n') return bad("an S line that does not end where it was measured to");
    for (char ch : text)
        if (ch == 0) return bad("a byte of the text that no item wrote");
    return fwrite(text.data(), 1, text.size(), stdout) == text.size();
}

int main(int argc, char **argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: gfa_check <case file>\n");
        return 2;
    }
    FILE *f = fopen(argv[1], "r");
    if (!f) {
        fprintf(stderr, "gfa_check: cannot open %s\n", argv[1]);
        return 2;
    }
    const bool ok = run(f);
    fclose(f);
    return ok ? 0 : 1;
}
