/*
 * gfa_chains_check — the item functions behind <prefix>.unitigs.gfa (disco_amd/csrc/disco_gfa_chains.h) on the host: the same header
 * the kernels include, built as plain C++, one "lane" after the other. tests/test_gfa_chains_host.py writes a case and compares the text.
 *   gfa_chains_check <case file>        -> the file's text on stdout
 * The case file, tokens separated by white space:
 *   n_reads has_file_index layout stride no_seq piece_bytes
 *       layout 0: rows of one stride of `stride` words; 1: two classes — 8-word rows for everybody, rows of `stride` words for the reads
 *       of more than 256 bases. piece_bytes: the chain S section is written in pieces of that many bytes (0: in one)
 *   per read: its bases (ACGT) [its file index, if has_file_index] skip      (skip 1: contained or inside a chain, no line of its own)
 *   n_composite then per composite edge: a b n_links, and n_links times: to offset orient      (read ids)
 *   n_edges then per edge that went into no composite edge: src dst orient offset
 * The sections are measured, scanned and written as disco_write_gfa_chains does; the chain S section piece by piece, every piece in a
 * buffer of exactly its size, item after item: an item must find its bytes unwritten and leave them written, and the piece full.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "../csrc/disco_gfa_chains.h"

static bool bad(const char *what)
{
    fprintf(stderr, "gfa_chains_check: %s\n", what);
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
    const uint64_t n = v[0], piece_bytes = v[5];
    const bool has_fi = v[1] != 0, classes = v[2] != 0, no_seq = v[4] != 0;
    const uint32_t stride = (uint32_t)v[3];
    if (stride == 0 || (classes && stride <= GFA_HEAD_WORDS)) return bad("stride");
    std::vector<uint16_t> len(n);
    std::vector<uint64_t> fi(has_fi ? n : 0);
    std::vector<uint32_t> ovf(n), long_ids;
    std::vector<uint8_t> skip(n);
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
        if (!get(v, 1)) return bad("a skip flag");
        skip[i] = v[0] != 0;
        ovf[i] = (uint32_t)long_ids.size();
        if (classes && len[i] > GFA_SHORT_MAX) long_ids.push_back((uint32_t)i);
    }
    /* the table: 2 bits a base, MSB first, A0 C1 G2 T3, unused bits zero */
    const uint32_t S = classes ? GFA_HEAD_WORDS : stride;
    std::vector<uint64_t> rows(n * S + 1, 0), full(long_ids.size() * (size_t)stride + 1, 0);
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

    if (!get(v, 1)) return bad("composite edges");
    std::vector<disco_chain_edge> comp(v[0]);
    std::vector<disco_chain_link> links;
    for (auto &c : comp) {
        if (!get(v, 3)) return bad("composite edge");
        if (v[0] >= n || v[1] >= n || v[2] < 2) return bad("a composite edge names no read, or has fewer than two links");
        c.a = v[0];
        c.b = v[1];
        c.n_links = (uint32_t)v[2];
        c.first_link = links.size();
        c.offset = 0;
        for (uint32_t j = 0; j < c.n_links; j++) {
            if (!get(v, 3)) return bad("link");
            const uint64_t from = j ? links.back().to : c.a;
            if (v[0] >= n || v[2] > 3 || v[1] >= len[from]) return bad("a link names no read or orientation, or begins behind the read before it");
            disco_chain_link l;
            l.to = (uint32_t)v[0];
            l.offset = (uint32_t)v[1];
            l.orient = (uint32_t)v[2];
            links.push_back(l);
            c.offset += l.offset;
        }
        c.orient = (links[c.first_link].orient & 2u) | (links.back().orient & 1u);
        if (links.back().to != c.b) return bad("the last link of a composite edge does not end at its b");
    }
    if (!get(v, 1)) return bad("edges");
    std::vector<GfaL> edges(v[0]);
    for (auto &e : edges) {
        if (!get(v, 4)) return bad("edge");
        if (v[0] >= n || v[1] >= n || v[2] > 3 || v[3] >= len[v[0]]) return bad("an edge names no read, orientation or offset");
        e.a = gfa_name(g, v[0]);
        e.b = gfa_name(g, v[1]);
        e.orient = (uint32_t)v[2];
        e.ovl = len[v[0]] - (uint32_t)v[3];
        e.nm = 0;
        e.has_nm = false;
    }

    /* measure, scan */
    std::vector<uint64_t> lsum(links.size() + 1, 0);
    for (size_t x = 0; x < links.size(); x++) lsum[x + 1] = lsum[x] + links[x].offset;
    GfuChains h;
    h.comp = comp.data();
    h.links = links.data();
    h.lsum = lsum.data();
    h.cplace = nullptr;
    h.n_comp = comp.size();
    h.no_seq = no_seq;
    const std::string header = GFA_HEADER;
    std::vector<uint64_t> splace(n + 1, header.size());
    for (uint64_t i = 0; i < n; i++) splace[i + 1] = splace[i] + (skip[i] ? 0u : gfa_s_bytes(gfa_name(g, i), len[i], no_seq));
    std::vector<uint64_t> cplace(comp.size() + 1, 0); /* (inside the chain S section, as on the device) */
    for (size_t k = 0; k < comp.size(); k++) cplace[k + 1] = cplace[k] + gfu_line(h, len.data(), k).bytes;
    h.cplace = cplace.data();
    const uint64_t chain_at = splace[n], chain_bytes = cplace[comp.size()];
    std::vector<uint64_t> lplace(edges.size() + 1, chain_at + chain_bytes);
    for (size_t i = 0; i < edges.size(); i++) lplace[i + 1] = lplace[i] + gfa_l_bytes(edges[i]);
    std::vector<uint64_t> klplace(comp.size() + 1, lplace[edges.size()]);
    for (size_t k = 0; k < comp.size(); k++) klplace[k + 1] = klplace[k] + gfu_l_bytes(gfu_l_of(g, h, k));
    std::vector<char> text(klplace[comp.size()], 0);
    header.copy(text.data(), header.size());

    /* the read S lines: gfa_s_write_kernel's and gfa_s_write_long_kernel's lanes behind the skip flag */
    const uint32_t W = no_seq ? 1u : S;
    for (uint64_t i = 0; i < n; i++)
        for (uint32_t w = 0; w < W; w++) {
            if (w >= gfa_s_items(len[i], no_seq) || skip[i]) continue;
            gfa_s_put(text.data() + splace[i], gfa_name(g, i), len[i], w, no_seq ? 0 : gfa_word(g, i, w), no_seq);
        }
    if (classes && !no_seq)
        for (size_t j = 0; j < long_ids.size(); j++)
            for (uint32_t w = GFA_HEAD_WORDS; w < stride; w++) {
                const uint64_t i = long_ids[j];
                if (w >= gfa_s_items(len[i], false) || skip[i]) continue;
                gfa_s_put(text.data() + splace[i], gfa_name(g, i), len[i], w, full[j * (size_t)stride + w], false);
            }
    /* the chain S section, piece by piece */
    const uint64_t step = piece_bytes ? piece_bytes : (chain_bytes ? chain_bytes : 1);
    for (uint64_t lo = 0; lo < chain_bytes; lo += step) {
        const uint64_t hi = lo + step < chain_bytes ? lo + step : chain_bytes, size = hi - lo;
        std::unique_ptr<char[]> piece(new char[size]()); /* (exactly its size: a store beyond it is the sanitizer's) */
        for (uint64_t t = 0; t < gfu_items(lo, hi); t++) {
            const uint64_t b = 16 * t, e = b + 16 < size ? b + 16 : size;
            for (uint64_t x = b; x < e; x++)
                if (piece[x]) return bad("an item found a byte of its own already written");
            gfu_item(g, h, lo, hi, t, piece.get());
            for (uint64_t x = b; x < e; x++)
                if (!piece[x]) return bad("an item left a byte of its own unwritten");
            for (uint64_t x = e; x < size; x++)
                if (piece[x]) return bad("an item wrote behind its bytes");
        }
        for (uint64_t x = 0; x < size; x++) text[chain_at + lo + x] = piece[x];
    }
    for (size_t k = 0; k < comp.size(); k++)
        if (text[chain_at + cplace[k + 1] - 1] != '\n') return bad("a chain S line that does not end where it was measured to");
    for (size_t i = 0; i < edges.size(); i++)
        if (gfa_l_put(text.data() + lplace[i], edges[i]) != text.data() + lplace[i + 1]) return bad("an L line of another number of bytes than measured");
    for (size_t k = 0; k < comp.size(); k++)
        if (gfu_l_put(text.data() + klplace[k], gfu_l_of(g, h, k)) != text.data() + klplace[k + 1]) return bad("the L lines of a composite edge of another number of bytes than measured");
    for (uint64_t i = 0; i < n; i++)
        if (!skip[i] && text[splace[i + 1] - 1] != '\n') return bad("an S line that does not end where it was measured to");
    for (char ch : text)
        if (ch == 0) return bad("a byte of the text that no item wrote");
    return fwrite(text.data(), 1, text.size(), stdout) == text.size();
}

int main(int argc, char **argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: gfa_chains_check <case file>\n");
        return 2;
    }
    FILE *f = fopen(argv[1], "r");
    if (!f) {
        fprintf(stderr, "gfa_chains_check: cannot open %s\n", argv[1]);
        return 2;
    }
    const bool ok = run(f);
    fclose(f);
    return ok ? 0 : 1;
}
