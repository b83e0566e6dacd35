/*
 * parsimple.h — the first step of the reference's SimplifyGraph on the graph the stage has just built.
 *
 * fullsimplify starts by running `parsimplify <edge file> <prefix>_<i>_ParSimpleEdges.txt <minOvl> <threads>` on every edge file
 * (SG/OverlapGraph.cpp:1051-1110) — unless all those files already exist, in which case it loads them and skips the step
 * (SG/OverlapGraph.cpp:1027-1049). parsimplify re-parses the text the stage wrote, contracts every chain of nodes with one way in
 * and one way out into a composite edge and removes weak dead ends, to a fixpoint (SG/OverlapGraphSimple.cpp:224-253:
 * contractParCompositeEdges, then { contractParCompositeEdges_Serial; removeParDeadEndNodes } until nothing changes).
 * write_par_simple does the same on the edges while they are still in memory and writes the files in parsimplify's format
 * (printEdge, SG/OverlapGraphSimple.cpp:658-690):
 *     src \t dst \t orient,offset,offset+len(dst),0,0 \t (read,orientation bit,offset)(…)…        source < destination
 * The result is the same SET of lines parsimplify writes for the same edge file (tests/test_host.py compares them sorted; the
 * reference's own line order depends on its container history, and a ring of absorbable nodes ends in a loop whose direction
 * the reference decides by pointer comparison). The ORDER of the lines in a file is this project's own and is a function of the
 * lines alone: by (smaller id, larger id), then — for parallel edges — by offset, number of links and orientation AS PRINTED, then by
 * the first link the line prints, which no two edges share. So every flow that arrives at the same edges writes the same bytes.
 */
#ifndef DISCO_PARSIMPLE_H_
#define DISCO_PARSIMPLE_H_

#include <cstdint>
#include <string>
#include <vector>

#include "disco_hip.h"
#include "fastx.h"
#include "writer.h"

namespace disco {

struct ParSimpleStats {
    uint64_t edges_in, edges_out, nodes_absorbed, dead_end_nodes, dead_end_edges, rounds;
};

/* the chains of the graph already contracted on the GPU (disco_contract_chains + disco_fetch_chains): the edges flagged in
 * `absorbed` are not loaded, the composite edges are; what remains for the host is the rings, the dead ends and the later rounds */
struct ChainSeed {
    const disco_chain_edge *comp = nullptr;
    uint64_t n_comp = 0;
    const disco_chain_link *links = nullptr;
    const uint8_t *absorbed = nullptr; /* [n_edges] */
};

/* edges / edge_file as for write_edges (file = connected component set, so no chain crosses files); min_ovl_simplify =
 * MinOverlap4SimplifyGraph (disco.cfg:38; edges below it are dropped at load, SG/OverlapGraphSimple.cpp:589) */
bool write_par_simple(const std::string &prefix, int n_files, const disco_edge *edges, size_t n_edges, const uint16_t *edge_file, const ReadSet &rs,
                      uint32_t min_ovl_simplify, int threads, std::string &err, ParSimpleStats *stats = nullptr, const FileTags *tags = nullptr,
                      const std::vector<std::string> *paths = nullptr /* explicit output file names, one per file */,
                      const uint8_t *marked = nullptr /* [n reads] nodes all of whose edges are in their file (flags 0 / 1 / 2 of the edge
                                                         lines, SG/OverlapGraphSimple.cpp:591-644); null: every node, as in buildG's files */,
                      const ChainSeed *seed = nullptr /* only with marked == null (the GPU contraction knows no marks) */);

/* ---- the same pass from the RESIDUE of a chain contraction on the GPU ------------------------------------------------------------
 * What the device hands over after disco_contract_chains is small: the simple edges no composite edge took
 * (disco_fetch_chain_residue) and one header per composite edge (disco_fetch_chains without links, disco_fetch_chain_first_edges for
 * their files). The pass — rings, dead ends, the later rounds to the fixpoint, the files' order — works on that graph with the
 * device's composite edges held as handles: everything the rules ask of an edge follows from its header (number of links, the offset
 * in either direction, the orientation at either end). No array has one entry per read: nodes are numbered by their place among the
 * reads the residue touches. The result is a description of every final line as a short list of pieces (disco_ps_edge /
 * disco_ps_piece, include/disco_hip.h), which disco_format_par_simple turns into text where the links are. Same files, same
 * ParSimpleStats as write_par_simple with a ChainSeed. */
struct ChainResidue {
    const disco_edge *edges = nullptr;      /* [n_edges] the residue                                                        */
    const uint16_t *edge_file = nullptr;    /* [n_edges] their files (null: file 0)                                         */
    uint64_t n_edges = 0;
    const disco_chain_edge *comp = nullptr; /* [n_comp] the composite edges' headers                                        */
    const uint16_t *comp_file = nullptr;    /* [n_comp] their files (null: file 0)                                          */
    uint64_t n_comp = 0;
    const disco_chain_link *comp_first = nullptr, *comp_last_rev = nullptr; /* [n_comp] the first link each prints, forward and turned
                                               round (disco_fetch_chain_end_links): what orders parallel edges with equal headers; null:
                                               taken from links                                                              */
    const disco_chain_link *links = nullptr; /* the composite edges' links: only to format on the host (no sink)            */
};
struct ParSimpleDescription {
    std::vector<disco_ps_edge> edges; /* printing direction, by file, in the files' line order */
    std::vector<disco_ps_piece> pieces;
    uint64_t reversed_pieces = 0; /* pieces of kind 2                 */
    uint32_t max_pieces = 0;      /* the largest piece count of an edge */
};
/* sink != null: the description goes there and no file is written (prefix / tags / paths are not used);
 * sink == null: res.links must be given, and the files are formatted and written here (disco_partext.h's functions, on the host) */
bool write_par_simple_residue(const std::string &prefix, int n_files, const ChainResidue &res, const ReadSet &rs, std::string &err, ParSimpleStats *stats = nullptr,
                              const FileTags *tags = nullptr, const std::vector<std::string> *paths = nullptr, ParSimpleDescription *sink = nullptr);

} // namespace disco
#endif
