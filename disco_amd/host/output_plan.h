/*
 * output_plan.h — who writes each file of a buildG run, decided once ("Who writes which file", is this header as a table).
 * Plain C++17: nothing of the GPU runtime, so disco_amd/bin/plan_check walks every combination on any machine (tests/test_output_plan_host.py).
 *   Options : what the command line and the parameter file say          Knobs : the environment, read in read_knobs() and nowhere else
 *   plan()  : for each of the five products None / Device / Host        demote() : Device -> Host after a soft error at run time
 * What follows from the routes — rows or edges needed on the host, the writer thread — is computed from the CURRENT routes, never stored.
 */
#ifndef DISCO_OUTPUT_PLAN_H_
#define DISCO_OUTPUT_PLAN_H_

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace disco {

/* buildG --gpus N: DISCO_DIST_GPU_TEXT=1 makes every rank write its share of the text files from its GPU. Measured with four ranks on ONE
 * device (profiles/dist_text.txt): from "Graph construction complete" to files closed the device path is slower at 5 M reads (each rank
 * pins a 256 MB staging ring for a few MB of text, one rank after the other) and faster at 50 M; the whole process is faster at both. Slower
 * at either size means opt-in; what one GPU and one link per rank gain is a measurement this pool cannot make. */
static const bool DIST_GPU_TEXT_DEFAULT = false;

/* buildG --par-simple on one GPU: the ParSimpleEdges files written from the device (disco_format_par_simple) instead of from the edges,
 * links and text fetched to the host. Measured against the commit before it, both in one session on one box, text output, three runs each
 * (profiles/par_simple_text.txt): from "fetch contained rows" through "partial simplification" 1.53-1.57 s -> 0.22 s at 5*10^7 x 150 bp
 * (45 M edges, 631 MB of lines) and 0.19-0.23 s -> 0.022 s on the 10 M-read metagenome graph; the process 2.7-3.5 s -> 1.0 s and (page
 * cache warm) 0.70-1.04 s -> 0.54-0.63 s. Lower at both shapes by more than either range: the default. DISCO_PAR_SIMPLE_GPU_TEXT=0 or
 * DISCO_PAR_SIMPLE_HOST_TEXT=1 keep the flow through the host. */
static const bool PAR_SIMPLE_GPU_TEXT_DEFAULT = true;

/* buildG --binary-out / --no-text on one GPU: DISCO_GPU_BINARY=1 has <prefix>_edges.bin and <prefix>_contained.bin written from the device
 * (disco_write_edge_records / disco_write_contained_records: no edge record and no contained row reaches the host, and with --binary-out the
 * text files keep their device path); 0 keeps the host writer (disco::write_binary). With --binary-out it is off unless asked for. With
 * --no-text the default is this constant, decided by the rule of profiles/par_simple_text.txt: on only when the device path's median is
 * lower at both measured shapes by more than the larger run-to-run range. Measured against the commit before and against this one with the
 * knob off, interleaved in one session on one box, three runs each (profiles/binary_records.txt): the laps from `wait for lengths + file
 * indices` to the end 0.963 -> 0.246 s at 5*10^7 x 150 bp (1.81 GB of edge records; larger range 0.033) and 0.343 -> 0.062 s on the 10 M-read
 * metagenome shape (0.052); the process 1.82 -> 1.00 s (0.32) and 0.79 -> 0.46 s (0.10). Lower at both by more than either range: the default. */
static const bool GPU_BINARY_NO_TEXT_DEFAULT = true;

struct Options {
    int gpus = 1, threads = 1;
    bool no_text = false, binary_out = false, par_simple = false, mpi_names = false, max_subs = false;
    int n_edge_files = 1, n_contained_files = 1; /* derived: count_files() */
    void count_files()
    {
        n_edge_files = mpi_names ? gpus * std::max(threads - 1, 1) : threads;
        n_contained_files = mpi_names ? gpus * threads : threads;
    }
};

/* Two readings, both kept as they always were: a FLAG is on when the variable is set to anything, "0" included; a TRI-state is its default
 * when unset, off when "0", on otherwise. */
enum Tri : signed char { TRI_UNSET = -1, TRI_OFF = 0, TRI_ON = 1 };
struct Knobs {
    bool host_text = false, host_contained_text = false, text_via_host = false, late_rows = false, host_row_sort = false; /* flags: DISCO_<NAME> */
    bool par_simple_host = false, par_simple_host_text = false;
    bool host_input = false, par_simple_env = false; /* not routes: DISCO_HOST_INPUT (the input stage), DISCO_PAR_SIMPLE (stands for --par-simple) */
    Tri gpu_binary = TRI_UNSET, par_simple_gpu_text = TRI_UNSET, dist_gpu_text = TRI_UNSET, dist_device_input = TRI_UNSET;
};
inline bool tri(Tri v, bool dflt) { return v == TRI_UNSET ? dflt : v == TRI_ON; }

/* the only place the routing variables are read (get: the environment, or plan_check's stand-in for it) */
inline Knobs read_knobs(char *(*get)(const char *) = ::getenv)
{
    auto flag = [&](const char *name) { return get(name) != nullptr; };
    auto tri3 = [&](const char *name) {
        const char *v = get(name);
        return !v ? TRI_UNSET : strcmp(v, "0") != 0 ? TRI_ON : TRI_OFF;
    };
    Knobs k;
    k.host_text = flag("DISCO_HOST_TEXT");
    k.host_contained_text = flag("DISCO_HOST_CONTAINED_TEXT");
    k.text_via_host = flag("DISCO_TEXT_VIA_HOST");
    k.late_rows = flag("DISCO_LATE_ROWS");
    k.host_row_sort = flag("DISCO_HOST_ROW_SORT");
    k.par_simple_host = flag("DISCO_PAR_SIMPLE_HOST");
    k.par_simple_host_text = flag("DISCO_PAR_SIMPLE_HOST_TEXT");
    k.host_input = flag("DISCO_HOST_INPUT");
    k.par_simple_env = flag("DISCO_PAR_SIMPLE");
    k.gpu_binary = tri3("DISCO_GPU_BINARY");
    k.par_simple_gpu_text = tri3("DISCO_PAR_SIMPLE_GPU_TEXT");
    k.dist_gpu_text = tri3("DISCO_DIST_GPU_TEXT");
    k.dist_device_input = tri3("DISCO_DIST_DEVICE_INPUT");
    return k;
}

enum Product { CONTAINED_TEXT = 0, EDGE_TEXT, CONTAINED_BIN, EDGES_BIN, PAR_SIMPLE, N_PRODUCTS };
enum class Maker : unsigned char { None, Device, Host };

struct OutputPlan {
    Options opt;
    Maker maker[N_PRODUCTS] = {Maker::None, Maker::None, Maker::None, Maker::None, Maker::None};
    /* fixed when the plan is made: a demotion comes too late to change them */
    bool chains_on_device = false; /* the chains of --par-simple contracted on the GPU (ranks: by rank 0, from the gathered edges) */
    bool rows_early = false;       /* the rows start to the host, grouped, while the edges are selected (if any read is contained) */
    bool rows_grouped = false;     /* the rows are fetched in their files' order (unless the library answers DISCO_E_UNSUPPORTED) */
    bool stream_edge_text = false; /* edge text formatted on the device goes straight into the files; else fetched, written by write_edge_text */

    bool device(Product p) const { return maker[p] == Maker::Device; }
    bool host(Product p) const { return maker[p] == Maker::Host; }
    /* a soft error (DISCO_E_NOMEM / DISCO_E_UNSUPPORTED), or nothing to format: the host writer takes the product over */
    void demote(Product p)
    {
        if (maker[p] == Maker::Device) maker[p] = Maker::Host;
    }
    bool edge_text_streamed() const { return device(EDGE_TEXT) && stream_edge_text; }
    /* the rows as host records: for host-formatted text and for the host writer of the binary file */
    bool rows_on_host() const { return (!opt.no_text && !device(CONTAINED_TEXT)) || (opt.binary_out && !device(CONTAINED_BIN)); }
    /* the contained-read files by a thread of their own beside the edge work — not beside the host writer of the binary file, which sorts the
     * rows in place; the ranks' rows arrive too late for it */
    bool contained_by_writer_thread() const { return opt.gpus == 1 && !opt.no_text && (!opt.binary_out || device(CONTAINED_BIN)) && !device(CONTAINED_TEXT); }
    /* the edges as host records: only for what still works on them there (binary side output, partial simplification, host-formatted text) */
    bool edges_on_host() const { return (opt.binary_out && !device(EDGES_BIN)) || (opt.par_simple && !device(PAR_SIMPLE)) || (!opt.no_text && !device(EDGE_TEXT)); }
};

inline OutputPlan plan(const Options &o, const Knobs &k)
{
    OutputPlan p;
    p.opt = o;
    auto by = [](bool wanted, bool on_device) { return !wanted ? Maker::None : on_device ? Maker::Device : Maker::Host; };
    const bool ps_files = o.par_simple && !o.mpi_names; /* (with --mpi-names the consumer simplifies per rank: no ParSimpleEdges files) */
    p.chains_on_device = ps_files && !k.par_simple_host;
    bool binary_dev = false, ps_dev = false, contained_dev, edges_dev;
    if (o.gpus == 1) {
        ps_dev = p.chains_on_device && !o.max_subs && !k.par_simple_host_text && tri(k.par_simple_gpu_text, PAR_SIMPLE_GPU_TEXT_DEFAULT);
        binary_dev = o.binary_out && tri(k.gpu_binary, o.no_text && GPU_BINARY_NO_TEXT_DEFAULT);
        /* with the binary files written from the device the rows are wanted on the host for host-formatted text only, and a --binary-out run
         * keeps the text path of a run without the flag */
        contained_dev = !o.no_text && (!o.binary_out || binary_dev) && !k.host_text && !k.host_contained_text;
        edges_dev = !o.no_text && !o.max_subs && o.n_edge_files <= 256 && !k.host_text;
        p.rows_early = !contained_dev && !(binary_dev && o.no_text) && !k.host_row_sort && !k.late_rows;
        p.rows_grouped = !k.host_row_sort;
        p.stream_edge_text = (!o.binary_out || binary_dev) && (!o.par_simple || ps_dev) && !k.text_via_host;
    } else {
        /* every rank writes its share of the text files from its GPU under the conditions of the single-GPU device path: text is wanted and
         * nothing else needs the records on the host (no binary side output, no partial simplification), exact overlaps */
        const bool ranks_text = tri(k.dist_gpu_text, DIST_GPU_TEXT_DEFAULT) && !o.no_text && !o.binary_out && !o.par_simple && !o.max_subs && !k.host_text && !k.text_via_host;
        contained_dev = ranks_text && !k.host_contained_text;
        edges_dev = ranks_text && o.n_edge_files <= 256;
        p.stream_edge_text = true;
    }
    p.maker[CONTAINED_TEXT] = by(!o.no_text, contained_dev);
    p.maker[EDGE_TEXT] = by(!o.no_text, edges_dev);
    p.maker[CONTAINED_BIN] = p.maker[EDGES_BIN] = by(o.binary_out, binary_dev);
    p.maker[PAR_SIMPLE] = by(ps_files, ps_dev);
    return p;
}

} // namespace disco
#endif
