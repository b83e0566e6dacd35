/*
 * partext_check — the item functions behind the ParSimpleEdges lines (disco_amd/csrc/disco_partext.h) on the host: the same header the
 * kernels include, built as plain C++, one "lane" after the other. tests/test_partext_host.py writes a case and compares the text.
 *   partext_check <case file>        -> the files' text on stdout, one behind the other; "offsets o_0 ... o_F" on stderr
 * The case file, numbers separated by white space:
 *   n_reads n_files has_file_index
 *   n_reads lengths              [n_reads file indices, if has_file_index]
 *   n_comp  then per composite edge: a b offset orient n_links first_link
 *   n_links then per link: to offset orient
 *   n_edges then per edge: src dst offset orient file first_piece n_pieces
 *   n_pieces then per piece: kind a offset orient
 * Measure -> scan -> write as disco_format_par_simple does, so the byte counts are checked against what is written.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../csrc/disco_partext.h"

static bool bad(const char *what)
{
    fprintf(stderr, "partext_check: %s\n", what);
    return false;
}

static bool run(FILE *f)
{
    unsigned long long n_reads, n_files, has_fi, v[7];
    auto get = [&](unsigned long long *out, int m) {
        for (int i = 0; i < m; i++)
            if (fscanf(f, "%llu", &out[i]) != 1) return false;
        return true;
    };
    if (!get(v, 3)) return bad("header");
    n_reads = v[0], n_files = v[1], has_fi = v[2];
    if (n_files == 0) return bad("no files");
    std::vector<uint16_t> len(n_reads);
    std::vector<uint64_t> fi(has_fi ? n_reads : 0);
    for (auto &x : len) {
        if (!get(v, 1)) return bad("lengths");
        x = (uint16_t)v[0];
    }
    for (auto &x : fi) {
        if (!get(v, 1)) return bad("file indices");
        x = v[0];
    }
    if (!get(v, 1)) return bad("composite edges");
    std::vector<disco_chain_edge> comp(v[0]);
    for (auto &c : comp) {
        if (!get(v, 6)) return bad("composite edge");
        c.a = v[0], c.b = v[1], c.offset = v[2], c.orient = (uint32_t)v[3], c.n_links = (uint32_t)v[4], c.first_link = v[5];
    }
    if (!get(v, 1)) return bad("links");
    std::vector<disco_chain_link> links(v[0]);
    for (auto &l : links) {
        if (!get(v, 3)) return bad("link");
        l.to = (uint32_t)v[0], l.offset = (uint32_t)v[1], l.orient = (uint32_t)v[2];
        if (l.to >= n_reads) return bad("a link names no read");
    }
    for (const auto &c : comp)
        if (c.n_links < 2 || c.first_link > links.size() || c.n_links > links.size() - c.first_link || c.a >= n_reads || c.b >= n_reads) return bad("a composite edge outside the links");
    if (!get(v, 1)) return bad("edges");
    std::vector<disco_ps_edge> edges(v[0]);
    for (auto &e : edges) {
        if (!get(v, 7)) return bad("edge");
        e.src = v[0], e.dst = v[1], e.offset = v[2], e.orient = (uint32_t)v[3], e.file = (uint32_t)v[4], e.first_piece = v[5], e.n_pieces = (uint32_t)v[6], e.pad = 0;
    }
    if (!get(v, 1)) return bad("pieces");
    std::vector<disco_ps_piece> pieces(v[0]);
    for (auto &p : pieces) {
        if (!get(v, 4)) return bad("piece");
        p.kind = (uint32_t)v[0], p.a = (uint32_t)v[1], p.offset = (uint32_t)v[2], p.orient = (uint32_t)v[3];
    }
    /* the two prefix tables, validated as the library validates them */
    std::vector<uint64_t> piece_link(pieces.size() + 1, 0), edge_item(edges.size() + 1, 0), first_item(n_files + 1, 0);
    for (size_t p = 0; p < pieces.size(); p++) {
        uint64_t nl = 1;
        if (pieces[p].kind == 0) {
            if (pieces[p].a >= n_reads) return bad("a piece names no read");
        } else if (pieces[p].kind <= 2) {
            if (pieces[p].a >= comp.size()) return bad("a piece names no composite edge");
            nl = comp[pieces[p].a].n_links;
        } else
            return bad("a piece of unknown kind");
        piece_link[p + 1] = piece_link[p] + nl;
    }
    uint32_t file = 0;
    for (size_t e = 0; e < edges.size(); e++) {
        const disco_ps_edge &x = edges[e];
        if (x.n_pieces == 0 || x.first_piece > pieces.size() || x.n_pieces > pieces.size() - x.first_piece) return bad("an edge's pieces lie outside the pieces");
        if (x.src >= n_reads || x.dst >= n_reads) return bad("an edge names no read");
        if (x.file >= n_files || x.file < file) return bad("files must ascend");
        edge_item[e + 1] = edge_item[e] + piece_link[x.first_piece + x.n_pieces] - piece_link[x.first_piece];
        for (; file < x.file; file++) first_item[file + 1] = edge_item[e];
    }
    const uint64_t n_items = edge_item.back();
    for (; file < n_files; file++) first_item[file + 1] = n_items;
    PsView g;
    g.edges = edges.data();
    g.pieces = pieces.data();
    g.edge_item = edge_item.data();
    g.piece_link = piece_link.data();
    g.comp = comp.data();
    g.links = links.data();
    g.len = len.data();
    g.file_index = has_fi ? fi.data() : nullptr;
    g.n_edges = edges.size();
    g.n_pieces = pieces.size();
    g.n_items = n_items;
    std::vector<uint64_t> place(n_items + 1, 0);
    for (uint64_t i = 0; i < n_items; i++) place[i + 1] = place[i] + ps_item_bytes(ps_item(g, i)); /* measure, scan */
    std::vector<char> text(place[n_items]);
    for (uint64_t i = 0; i < n_items; i++) { /* write: every item exactly the bytes it measured */
        if (place[i + 1] > text.size()) return bad("an item would write beyond the text");
        if (ps_put_item(text.data() + place[i], ps_item(g, i)) != text.data() + place[i + 1]) return bad("an item wrote another number of bytes than it measured");
    }
    fprintf(stderr, "offsets");
    for (uint64_t t = 0; t <= n_files; t++) fprintf(stderr, " %llu", (unsigned long long)place[first_item[t]]);
    fprintf(stderr, "\n");
    return fwrite(text.data(), 1, text.size(), stdout) == text.size();
}

int main(int argc, char **argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: partext_check <case file>\n");
        return 2;
    }
    FILE *f = fopen(argv[1], "r");
    if (!f) {
        fprintf(stderr, "partext_check: cannot open %s\n", argv[1]);
        return 2;
    }
    const bool ok = run(f);
    fclose(f);
    return ok ? 0 : 1;
}
