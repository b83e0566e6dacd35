/*
 * unitig_reads_check — the states, rounds and lines behind <prefix>.unitigs.reads (disco_amd/csrc/disco_unitig_reads.h) on the host: the
 * same header the kernels include, built as plain C++, one "lane" after the other. tests/test_unitig_reads_host.py writes a case and
 * compares the text.
 *   unitig_reads_check <case file>        -> the file's text on stdout, "rounds <r>" (the rounds that moved a read) on stderr
 * The case file, tokens separated by white space:
 *   n_reads has_file_index depth_only piece_lines        piece_lines: a section is written in pieces of that many lines (0: in one)
 *   per read: its length [its file index, if has_file_index] contained container orient start
 *       contained 1: the row its key decodes to (disco_contained_row: the containing read's id, orient 0..3, start); 0: three numbers
 *       that are not looked at
 *   n_composite then per composite edge: a b n_links, and n_links times: to offset orient      (read ids)
 * The stages are disco_write_unitig_reads': initial states, rounds of doubling between two arrays until one moves nobody (held to the
 * walk hop by hop, state for state), the links' places, the counts and their scans in link order, then every section measured,
 * scanned and written piece by piece, every piece in a buffer of exactly its size that its lines must fill. A row that names no read
 * and keys that do not settle in UTR_MAX_ROUNDS rounds are refused with a message, as the library refuses them.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "../csrc/disco_unitig_reads.h"

static bool bad(const char *what)
{
    fprintf(stderr, "unitig_reads_check: %s\n", what);
    return false;
}

/* one section: n_lines lines of bytes_of(i) bytes, line i written by put(i, at) -> the byte behind it; pieces of piece_lines lines */
static bool section(std::string &text, uint64_t n_lines, uint64_t piece_lines, const std::function<uint32_t(uint64_t)> &bytes_of,
                    const std::function<char *(uint64_t, char *)> &put)
{
    std::vector<uint64_t> place(n_lines + 1, 0);
    for (uint64_t i = 0; i < n_lines; i++) {
        const uint32_t b = bytes_of(i);
        if (b > 255) return bad("a line longer than its 8-bit measure");
        place[i + 1] = place[i] + b;
    }
    const uint64_t step = piece_lines ? piece_lines : (n_lines ? n_lines : 1);
    for (uint64_t lo = 0; lo < n_lines; lo += step) {
        const uint64_t hi = lo + step < n_lines ? lo + step : n_lines, size = place[hi] - place[lo];
        std::unique_ptr<char[]> piece(new char[size ? size : 1]()); /* (exactly its size: a store beyond it is the sanitizer's) */
        for (uint64_t i = lo; i < hi; i++) {
            if (place[i + 1] == place[i]) continue; /* (a skipped read: no line, no lane's store) */
            char *at = piece.get() + (place[i] - place[lo]);
            if (put(i, at) != piece.get() + (place[i + 1] - place[lo])) return bad("a line of another number of bytes than measured");
            if (at[place[i + 1] - place[i] - 1] != '\n') return bad("a line that does not end in a line end");
        }
        for (uint64_t x = 0; x < size; x++)
            if (!piece[x]) return bad("a byte of a piece that no line wrote");
        text.append(piece.get(), size);
    }
    return true;
}

static bool run(FILE *f)
{
    unsigned long long v[6];
    auto get = [&](unsigned long long *out, int m) {
        for (int i = 0; i < m; i++)
            if (fscanf(f, "%llu", &out[i]) != 1) return false;
        return true;
    };
    if (!get(v, 4)) return bad("header");
    const uint64_t n = v[0], piece_lines = v[3];
    const bool has_fi = v[1] != 0, depth_only = v[2] != 0;
    if (n >= (1ull << 31)) return bad("more than 2^31 reads");
    std::vector<uint16_t> len(n);
    std::vector<uint64_t> fi(has_fi ? n : 0);
    std::vector<uint8_t> contained(n);
    std::vector<uint64_t> state(n), other(n);
    uint64_t bad_keys = 0;
    struct Row {
        uint64_t y;
        uint32_t orient, start;
    };
    std::vector<Row> row(n);
    for (uint64_t i = 0; i < n; i++) {
        if (!get(v, 1) || v[0] == 0 || v[0] > 32767) return bad("a read's length");
        len[i] = (uint16_t)v[0];
        if (has_fi) {
            if (!get(v, 1)) return bad("a file index");
            fi[i] = v[0];
        }
        if (!get(v, 4) || v[2] > 3) return bad("a read's row");
        contained[i] = v[0] != 0;
        row[i] = Row{v[1], (uint32_t)v[2], (uint32_t)v[3]};
    }
    GfaReads g;
    g.rows = g.full = nullptr;
    g.ovf = g.long_ids = nullptr;
    g.len = len.data();
    g.file_index = has_fi ? fi.data() : nullptr;
    g.n = n;
    g.S = g.SL = 0;

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
    const uint64_t nl = links.size(), nk = comp.size();

    /* 1. the initial states, a lane per read (utr_init_kernel with the key decoded already) */
    for (uint64_t x = 0; x < n; x++) {
        UtrState s = utr_self(x);
        if (contained[x]) {
            if (row[x].y < n) s = utr_of_row(row[x].y, row[x].orient, row[x].start, len[row[x].y], len[x]);
            else bad_keys++;
        }
        state[x] = utr_pack(s);
    }
    if (bad_keys) {
        fprintf(stderr, "unitig_reads_check: %llu contained reads have a key that names no containing read\n", (unsigned long long)bad_keys);
        return false;
    }
    const std::vector<uint64_t> first = state;
    /* 2. rounds of doubling between two arrays, until one moves nobody */
    uint32_t rounds = 0;
    bool moving = true;
    uint64_t *cur = state.data(), *next = other.data();
    while (moving && rounds < UTR_MAX_ROUNDS) {
        uint32_t moved = 0;
        for (uint64_t x = 0; x < n; x++) moved |= utr_round(cur, next, len.data(), x);
        std::swap(cur, next);
        moving = moved != 0;
        rounds++;
    }
    if (moving) {
        fprintf(stderr, "unitig_reads_check: the containment keys do not settle in %u rounds of doubling: they hold a cycle\n", UTR_MAX_ROUNDS);
        return false;
    }
    fprintf(stderr, "rounds %u\n", rounds - 1);
    /* ... held to the walk, one hop after the other from the initial states */
    for (uint64_t x = 0; x < n; x++) {
        UtrState s = utr_unpack(first[x]);
        for (;;) {
            const UtrState t = utr_unpack(first[s.anc]);
            if (utr_is_root(t, s.anc)) break;
            s = utr_compose(s, t, len[s.anc], len[x]);
        }
        if (utr_pack(s) != cur[x]) return bad("doubling and the walk hop by hop disagree about a read");
        if (contained[s.anc]) return bad("a root that is contained");
    }
    /* 3. the links' places */
    std::vector<uint64_t> lsum(nl + 1, 0);
    for (uint64_t x = 0; x < nl; x++) lsum[x + 1] = lsum[x] + links[x].offset;
    GfuChains h;
    h.comp = comp.data();
    h.links = links.data();
    h.lsum = lsum.data();
    h.cplace = nullptr;
    h.n_comp = nk;
    h.no_seq = false;
    std::vector<uint32_t> cseg(n, UTR_NO_CHAIN), rcnt(n, 0);
    std::vector<uint64_t> cpos(n, 0), rbases(n, 0), kcnt(nl + 1, 0), kbases(nl + 1, 0);
    for (uint64_t x = 0; x < nl; x++) utr_place_link(h, x, cseg.data(), cpos.data());
    /* 4. the counts: every read to its root; the chains' totals from one scan in link order */
    for (uint64_t x = 0; x < n; x++) {
        const uint64_t r = utr_unpack(cur[x]).anc;
        rcnt[r] += 1;
        rbases[r] += len[x];
    }
    for (uint64_t x = 0; x < nl; x++) {
        uint64_t k;
        const bool in = utr_link_interior(h, x, &k);
        kcnt[x + 1] = kcnt[x] + (in ? rcnt[links[x].to] : 0u);
        kbases[x + 1] = kbases[x] + (in ? rbases[links[x].to] : 0ull);
    }
    UtrView view;
    view.state = cur;
    view.cseg = cseg.data();
    view.cpos = cpos.data();
    view.rcnt = rcnt.data();
    view.rbases = rbases.data();
    view.kcnt = kcnt.data();
    view.kbases = kbases.data();
    /* the skip flags of the S lines (gfu_mark_links_kernel, gfu_unmark_ends_kernel) */
    std::vector<uint8_t> skip(contained);
    for (uint64_t x = 0; x < nl; x++) skip[links[x].to] = 1;
    for (uint64_t k = 0; k < nk; k++) skip[comp[k].b] = contained[comp[k].b];
    /* 5. the text */
    std::string text = UTR_HEADER;
    if (!section(
            text, n, piece_lines, [&](uint64_t i) { return skip[i] ? 0u : utr_u_bytes(utr_u_of_read(g, view, i)); },
            [&](uint64_t i, char *at) { return utr_u_put(at, utr_u_of_read(g, view, i)); }))
        return false;
    if (!section(
            text, nk, piece_lines, [&](uint64_t k) { return utr_u_bytes(utr_u_of_chain(g, h, view, k)); },
            [&](uint64_t k, char *at) { return utr_u_put(at, utr_u_of_chain(g, h, view, k)); }))
        return false;
    if (!depth_only && !section(
                           text, n, piece_lines, [&](uint64_t x) { return utr_r_bytes(utr_r_of(g, view, x)); },
                           [&](uint64_t x, char *at) { return utr_r_put(at, utr_r_of(g, view, x)); }))
        return false;
    return fwrite(text.data(), 1, text.size(), stdout) == text.size();
}

int main(int argc, char **argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: unitig_reads_check <case file>\n");
        return 2;
    }
    FILE *f = fopen(argv[1], "r");
    if (!f) {
        fprintf(stderr, "unitig_reads_check: cannot open %s\n", argv[1]);
        return 2;
    }
    const bool ok = run(f);
    fclose(f);
    return ok ? 0 : 1;
}
