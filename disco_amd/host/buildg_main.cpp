/*
 * buildG — MI355X-native drop-in for DISCO's BuildGraph stage executable.
 *
 * Same command line and the same output files as the reference (/root/reference/src/BuildGraph/src/main.cpp:79-150,
 * runDisco.sh:200-245), so runDisco.sh works unmodified when this binary sits next to it:
 *     buildG [-pe f1,f2,...] [-se f1,...] -f <out prefix> -p <disco.cfg> [-t threads] [-m GB] [-w n] [--gpu id]
 *            [--gpus N [--same-device] [--mpi-names]]
 * -t sets the host thread count AND the number of <prefix>_<t>_parGraph.txt / _containedReads.txt files, as in the
 * reference. The graph itself is built on the GPU(s) through the C-ABI of libdisco_hip.so (include/disco_hip.h).
 * --gpus N is the replacement of buildG-MPI / buildG-MPIRMA (MPI/main.cpp:29-37, runDisco-MPI.sh:214-258): one rank per GPU
 * (a host thread each), reads and graph nodes range-partitioned, RCCL collectives inside the library; with --mpi-names the
 * files carry the <prefix>_<rank>_<thread>_ names those binaries write (MPI/OverlapGraph.cpp:127,370,419,518).
 */
#include <omp.h>

#include <sys/prctl.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <signal.h>
#include <fcntl.h>
#include <unistd.h>

#include <cerrno>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <fstream>
#include <functional>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "disco_hip.h"
#include "fastx.h"
#include "output_plan.h"
#include "parsimple.h"
#include "writer.h"

using Clock = std::chrono::steady_clock;
static double secs(Clock::time_point a) { return std::chrono::duration<double>(Clock::now() - a).count(); }

static void usage()
{
    std::cerr << "\nUsage: buildG [OPTION]...[PARAM]...\n"
              << "  -pe\tcomma separated paired-end (interleaved) read files, fasta/fastq[.gz]\n"
              << "  -se\tcomma separated single-end read files, fasta/fastq[.gz]\n"
              << "  -f\tprefix of all output files\n"
              << "  -p\tparameter file (MinOverlap4BuildGraph is read from it)\n"
              << "  -t\thost threads = number of partial graph files (default: all cores, at most 65534)\n"
              << "  -m\tmaximum host memory in GB (accepted for compatibility)\n"
              << "  --gpu\tfirst GPU to use (default 0)\n"
              << "  --gpus\tnumber of GPUs = ranks (default 1): reads and graph partitioned over them, RCCL exchanges\n"
              << "  --same-device\tall ranks on the GPU given by --gpu (in-process exchanges; single-GPU boxes)\n"
              << "  --partitioned-index\twith --gpus: the index stays hash-partitioned (buildG-MPIRMA's split hashData): lookups travel to the owners\n"
              << "  --mpi-names\tfile names <prefix>_<rank>_<thread>_... as written by buildG-MPI / buildG-MPIRMA (runDisco-MPI.sh)\n"
              << "  --par-simple\tprefix: also write <prefix>_<i>_ParSimpleEdges.txt, the output of the reference's parsimplify step on\n"
              << "\t\tevery edge file (fullsimplify then skips that step); DISCO_PAR_SIMPLE=1 in the environment derives the prefix\n"
              << "\t\tfrom -f the way runDisco.sh lays its directories out (<out>/graph/<name> -> <out>/assembly/<name>)\n"
              << "  --max-substitutions N\textension: accept overlaps / containments with up to N differing bases around an exact end-k-mer seed and\n"
              << "\t\twrite the count into the substitutions column (default 0 = the reference; parameter file key MaxSubstitutions4BuildGraph)\n"
              << "  --binary-out\talso write <prefix>_edges.bin / <prefix>_contained.bin (fixed 40-byte records, disco_amd/host/writer.h)\n"
              << "  --no-text\tbinary output only: leave the text edge / contained files empty (a consumer with the loader patch)\n"
              << "  --gfa\talso write <prefix>.gfa: the reduced graph as GFA 1.0 (S lines of all reads, L lines of the edges, C lines of the\n"
              << "\t\tcontained reads; names = the file indices of <prefix>_ReadIDMap.txt), formatted on the GPU; single GPU\n"
              << "  --gfa-no-seq\t--gfa with * in place of the bases\n"
              << "  --gfa-unitigs\talso write <prefix>.unitigs.gfa: the compacted graph as GFA 1.0 — every unbranched chain of reads one segment c<k>\n"
              << "\t\twith its merged bases, spelled on the GPU; no contained reads (--gfa has them); exact overlaps, single GPU;\n"
              << "\t\twith --gfa-no-seq beside it: * in place of the bases, and no <prefix>.gfa unless --gfa asks for it\n"
              << "  --unitig-reads\talso write <prefix>.unitigs.reads, the layout behind <prefix>.unitigs.gfa: a U line per segment (LN, reads, bases) and\n"
              << "\t\tan R line per read, contained ones included (segment, strand, 0-based start, length, the root of its containment\n"
              << "\t\twalk and the hops to it), resolved and formatted on the GPU; exact overlaps, single GPU\n"
              << "  --unitig-depth\t--unitig-reads with the U lines only: reads and bases per segment (depth = bases / LN)\n";
}

static std::vector<std::string> split(const std::string &s, char d)
{
    std::vector<std::string> v;
    std::stringstream ss(s);
    std::string item;
    while (std::getline(ss, item, d)) v.push_back(item);
    return v;
}

static std::string trim(const std::string &s)
{
    size_t a = s.find_first_not_of(" \t\r\n"), b = s.find_last_not_of(" \t\r\n");
    return a == std::string::npos ? std::string() : s.substr(a, b - a + 1);
}

/* whole-string unsigned number (decimal, 0x, 0 prefixes like the reference's stoull(..., 0)); false on anything else */
static bool parse_u64(const std::string &s, unsigned long long &out)
{
    const std::string t = trim(s);
    if (t.empty() || t[0] == '-') return false;
    errno = 0;
    char *end = nullptr;
    out = strtoull(t.c_str(), &end, 0);
    return errno == 0 && end && *end == '\0';
}

/* BG/main.cpp:152-176 : key = value lines; default 30 */
static bool read_min_overlap(const std::string &path, uint32_t &mo, std::string &err, uint32_t *mo_simplify = nullptr, uint32_t *max_subs = nullptr)
{
    std::ifstream f(path);
    if (!f.is_open()) return false;
    mo = 30;
    if (mo_simplify) *mo_simplify = 0; /* SG/Config.cpp: minOvl defaults to 0 */
    std::string line;
    while (std::getline(f, line)) {
        size_t eq = line.find('=');
        if (eq == std::string::npos) continue;
        auto tok = split(line, '=');
        if (tok.size() < 2) continue;
        if (trim(tok[0]) == "MinOverlap4BuildGraph") {
            unsigned long long v = 0;
            if (!parse_u64(tok[1], v) || v > 0xFFFFFFFFull) {
                err = "MinOverlap4BuildGraph = '" + trim(tok[1]) + "' in " + path + " is not a number";
                return true;
            }
            mo = (uint32_t)v;
        }
        /* extension key: the reference's parser looks for its own keys only and skips this line */
        if (max_subs && trim(tok[0]) == "MaxSubstitutions4BuildGraph") {
            unsigned long long v = 0;
            if (!parse_u64(tok[1], v) || v > 32767) {
                err = "MaxSubstitutions4BuildGraph = '" + trim(tok[1]) + "' in " + path + " is not a number in [0, 32767]";
                return true;
            }
            *max_subs = (uint32_t)v;
        }
        if (mo_simplify && trim(tok[0]) == "MinOverlap4SimplifyGraph") {
            unsigned long long v = 0;
            if (parse_u64(tok[1], v) && v <= 0xFFFFFFFFull) *mo_simplify = (uint32_t)v;
        }
    }
    return true;
}

static int die(const std::string &msg)
{
    std::cout << "\nError: " << msg << std::endl; /* the reference prints and exits 0 (BG/Common.h:64); we exit non-zero */
    return 2;
}

#define DISCO_CALL(ctx, expr)                                                              \
    do {                                                                                   \
        if ((expr) < 0) return die(std::string(#expr " : ") + disco_last_error(ctx));      \
    } while (0)

static const int GO_ON = -1; /* what a stage returns when the next one may run; anything else is the process's exit status */

struct Args {
    std::vector<std::string> pe, se;
    std::string prefix, cfg;
    int threads = omp_get_max_threads(), gpu = 0, gpus = 1;
    bool same_device = false, mpi_names = false, binary_out = false, no_text = false, partitioned_index = false;
    bool gfa = false, gfa_no_seq = false; /* <prefix>.gfa, with or without the bases */
    bool gfa_unitigs = false;             /* <prefix>.unitigs.gfa */
    bool unitig_reads = false, unitig_depth = false; /* <prefix>.unitigs.reads, whole or its U lines only (given both: whole) */
    std::string par_simple; /* prefix of the <prefix>_<i>_ParSimpleEdges.txt files, or empty */
    uint32_t min_overlap = 30, min_overlap_simplify = 0, max_subs = 0;
    std::vector<const char *> paths() const
    {
        std::vector<const char *> p;
        for (auto &f : pe) p.push_back(f.c_str());
        for (auto &f : se) p.push_back(f.c_str());
        return p;
    }
};

/* the command line, the parameter file and the checkpoint of an earlier run */
static int parse_args(int argc, char **argv, Args &a)
{
    long long max_subs_cli = -1; /* --max-substitutions (overrides MaxSubstitutions4BuildGraph of the parameter file) */
    bool gfa_cli = false;        /* --gfa itself */
    std::cout << "PRINTING ARGUMENTS\n";
    for (int i = 0; i < argc; i++) std::cout << argv[i] << ' ';
    std::cout << std::endl;
    if (argc == 1) {
        usage();
        return 0; /* BG/main.cpp:93-102 */
    }
    for (int i = 1; i < argc; i++) {
        std::string o = argv[i];
        bool bad = false;
        auto next = [&]() -> std::string {
            if (i + 1 < argc) return argv[++i];
            bad = true;
            return std::string();
        };
        auto num = [&](unsigned long long lo, unsigned long long hi) -> unsigned long long {
            unsigned long long v = 0;
            const std::string t = next();
            if (bad || !parse_u64(t, v) || v < lo || v > hi) {
                bad = true;
                std::cerr << "Option " << o << " needs a number in [" << lo << ", " << hi << "]" << (t.empty() ? "" : ", got '" + t + "'") << "\n";
            }
            return v;
        };
        if (o == "-pe") for (auto &f : split(next(), ',')) a.pe.push_back(f);
        else if (o == "-se") for (auto &f : split(next(), ',')) a.se.push_back(f);
        else if (o == "-f") a.prefix = next();
        else if (o == "-t") a.threads = (int)num(1, 65534); /* one partial graph file per thread: 16-bit file index */
        else if (o == "-w") (void)num(0, ~0ull);
        else if (o == "-m") (void)num(0, ~0ull);
        else if (o == "-p") a.cfg = next();
        else if (o == "--gpu") a.gpu = (int)num(0, 1023);
        else if (o == "--gpus") a.gpus = (int)num(1, 64);
        else if (o == "--same-device") a.same_device = true;
        else if (o == "--partitioned-index") a.partitioned_index = true;
        else if (o == "--mpi-names") a.mpi_names = true;
        else if (o == "--par-simple") a.par_simple = next();
        else if (o == "--max-substitutions") max_subs_cli = (long long)num(0, 32767);
        else if (o == "--binary-out") a.binary_out = true;
        else if (o == "--no-text") a.binary_out = a.no_text = true;
        else if (o == "--gfa") gfa_cli = true;
        else if (o == "--gfa-no-seq") a.gfa_no_seq = true;
        else if (o == "--gfa-unitigs") a.gfa_unitigs = true;
        else if (o == "--unitig-reads") a.unitig_reads = true;
        else if (o == "--unitig-depth") a.unitig_depth = true;
        else {
            usage();
            if (o == "-h" || o == "--help") return 0;
            std::cerr << "Unknown option: " << o << "\n\n";
            return 1; /* BG/main.cpp:133-148 */
        }
        if (bad) {
            usage();
            return 1;
        }
    }
    a.gfa = gfa_cli || (a.gfa_no_seq && !a.gfa_unitigs); /* alone, --gfa-no-seq means --gfa; beside --gfa-unitigs it is that file's */
    if (a.gfa_unitigs && a.gpus > 1) {
        std::cerr << "--gfa-unitigs writes the graph of one GPU: with --gpus " << a.gpus << " every rank holds its share only, run it without --gpus." << std::endl;
        return 1;
    }
    const char *layout = a.unitig_reads ? "--unitig-reads" : a.unitig_depth ? "--unitig-depth" : nullptr;
    if (layout && a.gpus > 1) {
        std::cerr << layout << " writes the graph of one GPU: with --gpus " << a.gpus << " every rank holds its share only, run it without --gpus." << std::endl;
        return 1;
    }
    if (a.gfa && a.gpus > 1) {
        std::cerr << "--gfa writes the graph of one GPU: with --gpus " << a.gpus << " every rank holds its share only, run it without --gpus." << std::endl;
        return 1;
    }
    std::string cfg_err;
    if (!read_min_overlap(a.cfg, a.min_overlap, cfg_err, &a.min_overlap_simplify, &a.max_subs)) {
        std::cerr << "Unable to open parameter file: " << a.cfg << std::endl;
        return 1; /* BG/main.cpp:157-160 */
    }
    if (!cfg_err.empty()) {
        std::cerr << cfg_err << std::endl;
        return 1;
    }
    std::cout << "MinOverlap4BuildGraph = " << a.min_overlap << std::endl;
    disco::set_writer_threads(a.threads);
    if (max_subs_cli >= 0) a.max_subs = (uint32_t)max_subs_cli;
    if (a.gfa_unitigs && a.max_subs) {
        std::cerr << "--gfa-unitigs spells every chain from reads that overlap exactly: with " << a.max_subs << " substitutions allowed (--max-substitutions, "
                  << "MaxSubstitutions4BuildGraph) the reads of a chain disagree about its bases. Use --gfa." << std::endl;
        return 1;
    }
    if (layout && a.max_subs) {
        std::cerr << layout << " places every read on chains spelled from reads that overlap exactly: with " << a.max_subs << " substitutions allowed (--max-substitutions, "
                  << "MaxSubstitutions4BuildGraph) the reads of a chain disagree about its bases. Use --gfa." << std::endl;
        return 1;
    }
    if (a.max_subs)
        std::cout << "MaxSubstitutions4BuildGraph = " << a.max_subs << " (extension: overlaps and containments may differ in that many bases around an exact "
                  << "end-k-mer seed; the reference compares exactly)" << std::endl;
    bool ccr = false, gc = false;
    disco::read_checkpoint(a.prefix, ccr, gc);
    if (gc) { /* BG/main.cpp:48-52 */
        std::cout << "Graph already exists. Using previously built graph...\nExiting graph construction." << std::endl;
        return 0;
    }
    return GO_ON;
}

/* two-pass verify for read sets of mixed lengths (metagenomes: most reads contained): same files, fewer candidate-row fetches;
 * only the diagnostic k-mer-hit count in the log then counts the compared candidates */
static disco_params make_params(const Args &a)
{
    return disco_params{a.min_overlap, 4, DISCO_FLAG_SEEDED_KMER | (getenv("DISCO_EXACT_COUNTERS") ? 0u : DISCO_FLAG_TWO_PASS_VERIFY), a.max_subs};
}

/* a thread that is joined when its holder goes away (stop: told to end first) — an early return must not leave a joinable thread behind */
struct JoinOnExit {
    std::thread t;
    std::atomic<bool> *stop = nullptr;
    ~JoinOnExit()
    {
        if (stop) stop->store(true);
        if (t.joinable()) t.join();
    }
};

/* descriptors that are closed when their holder goes away, whichever way */
struct Fds {
    std::vector<int> fd;
    Fds() = default;
    Fds(const Fds &) = delete;
    Fds &operator=(const Fds &) = delete;
    int *data() { return fd.data(); }
    void close_all()
    {
        for (int &f : fd)
            if (f >= 0) {
                close(f);
                f = -1;
            }
    }
    ~Fds() { close_all(); }
};

/* Watchdog of the multi-rank stage (bench.py has its twin): every rank thread names the call it is in; when NO rank has moved for
 * DISCO_WATCHDOG_S seconds (default 900; 0: off) — a collective one rank never entered, a link that went away — the process says
 * where every rank stands and exits non-zero. Never a re-exec, never a silent hang: runDisco.sh does not check the status, but
 * the missing GC=Complete line makes the next run start over. */
enum { ST_START = 0, ST_COMM_INIT, ST_INGEST, ST_INGEST_FETCH, ST_HOST_INPUT, ST_UPLOAD, ST_FRONT_OF_PASS, ST_PASS, ST_FETCH_CONTAINED, ST_FETCH_EDGES, ST_FORMAT_CONTAINED, ST_WRITE_CONTAINED, ST_FORMAT_EDGES, ST_WRITE_EDGES, ST_DONE };
static const char *const kStage[] = {"start", "disco_comm_init", "disco_dist_ingest_fasta", "disco_dist_ingest_fetch", "the host input stage (between the rank threads)",
                                     "disco_dist_upload_reads", "front of disco_dist_run_graph (never entered it)", "disco_dist_run_graph",
                                     "disco_fetch_contained", "disco_fetch_edges", "disco_dist_format_contained", "disco_write_contained_text (its contained-read files)",
                                     "disco_dist_format_edges", "disco_write_edge_text (its edge files)", "done"};

/* Everything the stages of one run share. THE ORDER OF THE MEMBERS SECURES PROPERTY 1: members die in reverse order of declaration, and the
 * four thread holders come last — so on every way out of main(), early returns included, every thread (ingest fetch, contained writer,
 * context releaser, watchdog) is joined before anything it references (the read set, the rows, the atomics) goes away. */
struct Job {
    Args a;
    disco::Knobs knobs;
    disco::OutputPlan plan;
    bool verbose = false;
    Clock::time_point t_main, t0, t1; /* process start; start of the running stage; start of the running lap */
    disco::ReadSet rs;
    std::string err;
    bool ingested = false;      /* the input stage ran on the device(s): the reads are in place there */
    disco_ctx *ctx1 = nullptr;  /* the single-GPU context, created in the input stage when the device stage is tried */
    std::vector<disco_ctx *> ctx; /* the ranks' contexts */
    unsigned char uid[DISCO_UNIQUE_ID_BYTES];
    bool comm_joined = false; /* (RCCL: the ranks joined the communicator in front of the device input stage) */
    std::vector<std::atomic<int>> stage; /* per rank: the call it is in (ST_*) */
    std::atomic<bool> ranks_done{false};
    std::atomic<bool> wd_paused{false}; /* the host stage runs on the main thread: no rank moves, and nobody waits for one */
    std::atomic<int> ingest_fetch_rc{0};
    disco::FileTags etags, ctags;
    uint64_t n_cont = 0, e_pre = 0, e_out = 0;
    double t_graph = 0, t_h2d = 0;
    std::vector<disco_contained_row> rows;
    bool rows_grouped = false; /* rows already are in the contained-read files' order (disco_fetch_contained_grouped) */
    std::unique_ptr<disco_edge[]> edges;
    std::unique_ptr<uint16_t[]> edge_file;
    std::unique_ptr<uint16_t[]> edge_subs; /* substitutions per edge (third number of an edge line); stays null with exact overlaps */
    std::unique_ptr<char[]> edge_text;     /* the edge lines, formatted on the GPU and fetched (single GPU, exact overlaps) */
    std::vector<uint64_t> edge_text_off;
    std::vector<disco_chain_edge> ch_comp; /* the chains of the reduced graph, contracted on the GPU (--par-simple) */
    std::unique_ptr<disco_chain_link[]> ch_links;
    std::unique_ptr<uint8_t[]> ch_absorbed;
    bool contained_ok = true; /* the writer thread's result */
    std::string contained_err;
    JoinOnExit ingest_fetch, watchdog{{}, &ranks_done}, contained_writer, ctx_releaser;

    void lap(const char *what)
    {
        if (verbose) fprintf(stderr, "[disco host] %-28s %.3f s\n", what, secs(t1));
        t1 = Clock::now();
    }
    /* file indices for the device's formatters; null when no record was filtered: file index = read id + 1 */
    const uint64_t *ids() const { return rs.total_records == rs.size() ? nullptr : rs.file_index.data(); }
    bool join_ingest_fetch()
    {
        if (ingest_fetch.t.joinable()) ingest_fetch.t.join();
        return ingest_fetch_rc.load() >= 0;
    }
};

/* what a device input stage reports about the read set (disco_ingest_info / disco_dist_ingest_info) and the files */
template <class Info>
static void fill_from_ingest(Job &J, const Info &ii, const std::vector<const char *> &paths, const disco_ingest_file *files)
{
    disco::ReadSet &rs = J.rs;
    rs.n_reads = ii.n_reads;
    rs.stride_words = ii.stride_words;
    rs.total_records = ii.total_records;
    rs.too_long = ii.too_long;
    rs.shortest = ii.shortest;
    rs.longest = ii.longest;
    for (size_t i = 0; i < paths.size(); i++) {
        disco::FileRange fr;
        fr.name = paths[i];
        fr.paired = i < J.a.pe.size();
        fr.first_index = files[i].first_index;
        fr.last_index = files[i].last_index;
        fr.good = files[i].good;
        fr.bad = files[i].bad;
        rs.files.push_back(fr);
    }
    J.ingested = true;
}

static void on_ranks(int gpus, const std::function<void(int)> &fn)
{
    std::vector<std::thread> th;
    for (int r = 0; r < gpus; r++) th.emplace_back(fn, r);
    for (auto &t : th) t.join();
}

/* the ranks' contexts, the communicator (in-process: joined here; RCCL: its id) and the watchdog; "" or what went wrong */
static std::string make_ranks(Job &J)
{
    const Args &a = J.a;
    const int gpus = a.gpus;
    const disco_params prm0 = make_params(a);
    J.ctx.assign((size_t)gpus, nullptr);
    for (int r = 0; r < gpus; r++)
        if (disco_create(a.same_device ? a.gpu : a.gpu + r, &prm0, &J.ctx[(size_t)r]) < 0)
            return std::string("disco_create (rank ") + std::to_string(r) + "): " + disco_last_error(nullptr) +
                   (a.same_device ? "" : " — one GPU per rank is needed; --same-device runs all ranks on one GPU");
    if (a.same_device) {
        if (disco_comm_init_local(J.ctx.data(), gpus) < 0) return "disco_comm_init_local failed";
    } else if (disco_comm_unique_id(J.uid, sizeof J.uid) < 0)
        return std::string("disco_comm_unique_id: ") + disco_last_error(nullptr);
    const long wd_s = getenv("DISCO_WATCHDOG_S") ? atol(getenv("DISCO_WATCHDOG_S")) : 900;
    J.watchdog.t = std::thread([&J, gpus, wd_s]() {
        if (wd_s <= 0) return;
        std::vector<int> last((size_t)gpus, -1);
        auto moved_at = Clock::now();
        while (!J.ranks_done.load()) {
            std::this_thread::sleep_for(std::chrono::milliseconds(200));
            bool moved = J.wd_paused.load();
            for (int r = 0; r < gpus; r++) {
                const int x = J.stage[(size_t)r].load();
                moved = moved || x != last[(size_t)r];
                last[(size_t)r] = x;
            }
            if (moved) moved_at = Clock::now();
            else if (secs(moved_at) > (double)wd_s) {
                std::cout << "\nError: no rank has made progress for " << wd_s << " seconds:";
                for (int r = 0; r < gpus; r++) std::cout << " rank " << r << " in " << kStage[last[(size_t)r]] << ";";
                std::cout << " giving up (DISCO_WATCHDOG_S sets the patience)." << std::endl;
                _exit(3);
            }
        }
    });
    return "";
}

/* The input stage on the GPU (disco_ingest_fasta: the files travel to HBM as text; records, read filter, ids and the 2-bit rows are
 * kernels) for one GPU and plain FASTA / FASTQ files of the common form; DISCO_E_UNSUPPORTED (.gz, a '>' inside a line of a FASTA
 * file, irregularly wrapped long records, unreadable or empty files) leaves everything to the host stage, which follows the reference's getline calls
 * literally and prints its messages. DISCO_HOST_INPUT=1: the host stage always. */
static int input_single_device(Job &J)
{
    const Args &a = J.a;
    disco::ReadSet &rs = J.rs;
    const disco_params prm0 = make_params(a);
    if (disco_create(a.gpu, &prm0, &J.ctx1) < 0) return die(std::string("disco_create: ") + disco_last_error(nullptr));
    disco_ctx *ctx1 = J.ctx1;
    if (getenv("DISCO_VERBOSE")) fprintf(stderr, "[disco host] process start to context ready   %.3f s\n", secs(J.t_main));
    const std::vector<const char *> paths = a.paths();
    std::vector<disco_ingest_file> ifiles(paths.size());
    disco_ingest_info ii;
    const int irc = disco_ingest_fasta(ctx1, paths.data(), (int)paths.size(), (uint32_t)a.threads, &ii, ifiles.data());
    if (irc == DISCO_OK) {
        fill_from_ingest(J, ii, paths, ifiles.data());
        /* lengths and file indices of the reads come to the host on a thread of their own while the graph is built: only the
         * writers need them */
        J.ingest_fetch.t = std::thread([&rs, &rc = J.ingest_fetch_rc, ctx1, n = ii.n_reads]() {
            const auto tf = Clock::now();
            /* (first touch by two threads: value-initialising 500 MB in one took 0.12 s, which the graph pass does not cover) */
            std::thread zl([&rs, n]() { rs.len.resize(n); });
            rs.file_index.resize(n);
            zl.join();
            const double tz = secs(tf);
            rc = disco_ingest_fetch(ctx1, rs.len.data(), rs.file_index.data());
            if (getenv("DISCO_VERBOSE")) fprintf(stderr, "[disco host] lengths + file indices to the host  %.3f s (of which first touch %.3f)\n", secs(tf), tz);
        });
        if (getenv("DISCO_VERBOSE"))
            fprintf(stderr, "[disco host] input stage on the GPU: files into HBM %.3f s, records + filter + ids + rows %.3f s\n", ii.read_s, ii.device_s);
    } else if (irc != DISCO_E_UNSUPPORTED)
        return die(std::string("disco_ingest_fasta: ") + disco_last_error(ctx1));
    else if (getenv("DISCO_VERBOSE"))
        fprintf(stderr, "[disco host] %s\n", disco_last_error(ctx1));
    return GO_ON;
}

/* --gpus N: the contexts, the communicator and the watchdog exist BEFORE the input stage, because every rank reads its share of the
 * files itself (disco_dist_ingest_fasta: the bytes of the files laid end to end, cut into N shares; records, filter and rows on the
 * rank's GPU, rows of other ranks' home ranges sent to their owners). DISCO_E_UNSUPPORTED — on every rank alike: a .gz name (BGZF too, unless DISCO_DIST_BGZF=1 asks the ranks to decode it), a '>'
 * inside a line, an irregularly wrapped long record, an unreadable file — leaves the job to the host stage, inside the same
 * run and on the same contexts. Asked for with DISCO_DIST_DEVICE_INPUT=1 (input_stage: why not by default); DISCO_HOST_INPUT=1: the host stage always. */
static int input_ranks_devices(Job &J)
{
    const Args &a = J.a;
    disco::ReadSet &rs = J.rs;
    const int gpus = a.gpus;
    if (const std::string e = make_ranks(J); !e.empty()) return die(e);
    const std::vector<const char *> paths = a.paths();
    /* reader threads per rank: all ranks together stay within 16 (one GPU: six keep the ring full, buildg's host has 16 cores). The
     * right figure for N links is a measurement nobody can make on this pool (its ranks share one device and one link). */
    const uint32_t readers = (uint32_t)std::max(1, std::min(a.threads, 16) / gpus);
    std::vector<int> irc((size_t)gpus, 0);
    std::vector<disco_dist_ingest_info> dii((size_t)gpus);
    std::vector<std::vector<disco_ingest_file>> ifiles((size_t)gpus, std::vector<disco_ingest_file>(paths.size()));
    on_ranks(gpus, [&](int r) {
        disco_ctx *c = J.ctx[(size_t)r];
        J.stage[(size_t)r].store(ST_COMM_INIT);
        if (!a.same_device && disco_comm_init(c, J.uid, gpus, r) < 0) {
            /* the other ranks wait for this one inside a collective: there is nothing to unwind to */
            std::cout << "\nError (rank " << r << "): disco_comm_init: " << disco_last_error(c) << std::endl;
            _exit(2);
        }
        J.stage[(size_t)r].store(ST_INGEST);
        irc[(size_t)r] = disco_dist_ingest_fasta(c, paths.data(), (int)paths.size(), readers, &dii[(size_t)r], ifiles[(size_t)r].data());
    });
    J.comm_joined = true;
    bool all_ok = true, all_declined = true;
    for (int r = 0; r < gpus; r++) {
        all_ok = all_ok && irc[(size_t)r] == DISCO_OK;
        all_declined = all_declined && irc[(size_t)r] == DISCO_E_UNSUPPORTED;
    }
    if (all_ok) {
        rs.len.resize(dii[0].n_reads);
        rs.file_index.resize(dii[0].n_reads);
        /* the ranks' home ranges, one behind the other, are the job's reads: lengths and file indices for _ReadIDMap.txt and the writers */
        on_ranks(gpus, [&](int r) {
            J.stage[(size_t)r].store(ST_INGEST_FETCH);
            const disco_dist_ingest_info &d = dii[(size_t)r];
            if (d.home_hi > d.home_lo) irc[(size_t)r] = disco_dist_ingest_fetch(J.ctx[(size_t)r], rs.len.data() + d.home_lo, rs.file_index.data() + d.home_lo);
        });
        for (int r = 0; r < gpus; r++)
            if (irc[(size_t)r] < 0) return die(std::string("disco_dist_ingest_fetch: ") + disco_last_error(J.ctx[(size_t)r]));
        fill_from_ingest(J, dii[0], paths, ifiles[0].data());
        if (getenv("DISCO_VERBOSE"))
            for (int r = 0; r < gpus; r++)
                fprintf(stderr, "[disco host] input stage on the GPU of rank %d: its bytes into HBM %.3f s, records + filter + ids + rows + exchange %.3f s\n", r, dii[(size_t)r].read_s,
                        dii[(size_t)r].device_s);
    } else if (!all_declined) {
        for (int r = 0; r < gpus; r++)
            if (irc[(size_t)r] != DISCO_OK && irc[(size_t)r] != DISCO_E_UNSUPPORTED) return die(std::string("disco_dist_ingest_fasta (rank ") + std::to_string(r) + "): " + disco_last_error(J.ctx[(size_t)r]));
        return die("disco_dist_ingest_fasta: the ranks disagree about the input");
    } else if (getenv("DISCO_VERBOSE"))
        fprintf(stderr, "[disco host] %s\n", disco_last_error(J.ctx[0]));
    for (auto &st : J.stage) st.store(ST_HOST_INPUT);
    return GO_ON;
}

/* the reads: on the single device, on the ranks' devices, or on the host; then what the reference prints about them and _ReadIDMap.txt */
static int input_stage(Job &J)
{
    const Args &a = J.a;
    disco::ReadSet &rs = J.rs;
    J.t0 = Clock::now();
    /* the packed reads go into ordinary memory: pinning 2 GB (hipHostMalloc) takes 0.5 s, which the upload then wins back only
     * 0.09 s of (0.09 against 0.18 s at config 3); DISCO_PINNED_READS=1 pins them all the same */
    disco::HostAlloc pinned;
    if (getenv("DISCO_PINNED_READS")) {
        pinned.alloc = disco_host_alloc;
        pinned.free = disco_host_free;
    }
    int rc = GO_ON;
    if (a.gpus == 1 && !J.knobs.host_input) rc = input_single_device(J);
    /* Measured (profiles/dist_ingest.txt): four ranks on ONE device, 5 M reads — the device stage on the ranks is not faster than the host
     * stage there (the ranks share one GPU and one link), so the host stage stays the default under --gpus N and
     * DISCO_DIST_DEVICE_INPUT=1 asks for the device stage; what one GPU per rank gains is a measurement this pool cannot make. */
    if (a.gpus > 1 && disco::tri(J.knobs.dist_device_input, false) && !J.knobs.host_input) rc = input_ranks_devices(J);
    if (rc != GO_ON) return rc;
    J.wd_paused.store(true); /* PROPERTY 3: the watchdog is paused while the host input stage runs (graph_ranks lets it go on) */
    if (!J.ingested && !disco::load_reads(a.pe, a.se, a.min_overlap, a.threads, rs, J.err, pinned)) return die(J.err);
    for (auto &fr : rs.files) {
        std::cout << "File name: " << fr.name << "\n"
                  << "  " << fr.good << " good reads in current dataset.\n  " << fr.bad << " bad reads in current dataset.\n  "
                  << (fr.good + fr.bad) << " total reads in current dataset.\n";
    }
    std::cout << "Shortest read length in all datasets: " << rs.shortest << "\n Longest read length in all datasets: " << rs.longest << std::endl;
    if (rs.too_long)
        std::cout << "Warning: " << rs.too_long << " reads longer than 32767 bp were dropped (15-bit length field of the index records, "
                  << "BG/HashTable.cpp:531); the reference would keep them." << std::endl;
    if (rs.size() == 0) return die("No reads found in the read files provided! Please check if the filename(s) and path(s) are correct.");
    if (!disco::write_read_id_map(a.prefix, rs, J.err)) return die(J.err);
    std::cout << "Function readDataset() finished in " << secs(J.t0) << " Seconds." << std::endl;
    return GO_ON;
}

/* DISCO_PAR_SIMPLE=1 stands for --par-simple with the prefix runDisco.sh:166-167 implies: <out>/graph/<name> and <out>/assembly/<name> */
static void par_simple_prefix_from_layout(Args &a)
{
    const std::string &prefix = a.prefix;
    const size_t at = prefix.rfind("/graph/");
    std::string base, name;
    bool found = false;
    if (at != std::string::npos) {
        base = prefix.substr(0, at + 1);
        name = prefix.substr(at + 7);
        found = true;
    } else if (prefix.compare(0, 6, "graph/") == 0) { /* relative to the output directory itself */
        name = prefix.substr(6);
        found = true;
    }
    if (found) {
        a.par_simple = base + "assembly/" + name;
        (void)mkdir((base + "assembly").c_str(), 0777); /* runDisco.sh keeps an existing assembly directory ("Will continue previous run") */
    } else
        std::cout << "DISCO_PAR_SIMPLE: the output prefix is not <out>/graph/<name>; use --par-simple <prefix>" << std::endl;
}

static void print_contained_counts(const Job &J)
{
    std::cout << "\n" << (J.rs.size() - J.n_cont) << " Non-contained reads. (Keep as is)\n"
              << J.n_cont << " contained reads. (Need to change their mate-pair information)" << std::endl;
}

/* "Graph construction complete<where>." with the counters, an extra line of the ranks', the caller's "Function buildOverlapGraph() ..." line */
static void print_graph_summary(const Job &J, const std::string &where, uint64_t probes, uint64_t kmer_hits, uint64_t cap_bind_sites, uint64_t asymmetric_pairs,
                                const std::string &regime_line, const std::string &finished)
{
    std::cout << "Graph construction complete" << where << ".\n"
              << "  overlaps (pre-reduction) : " << J.e_pre << "\n  edges after reduction    : " << J.e_out << "\n  k-mer probes             : " << probes
              << "\n  k-mer hits               : " << kmer_hits << "\n  cap_bind_sites           : " << cap_bind_sites
              << "\n  asymmetric_pairs         : " << asymmetric_pairs << "\n"
              << regime_line << finished << std::endl;
    if (!J.a.max_subs && (cap_bind_sites || asymmetric_pairs))
        std::cout << "Note: this input is in the order-dependent regime of the reference (edge cap per k-mer reached or overlaps found from one "
                     "side only); the reference's own result varies with its thread count here."
                  << std::endl;
}

static void print_par_simple_summary(const Job &J, const disco::ParSimpleStats &ps)
{
    std::cout << "Partial simplification (the reference's parsimplify step) on the resident graph: " << ps.edges_in << " edges -> " << ps.edges_out << " ("
              << ps.nodes_absorbed << " nodes absorbed into composite edges, " << ps.dead_end_nodes << " dead-end nodes, " << ps.rounds << " rounds); files "
              << J.a.par_simple << "_<i>_ParSimpleEdges.txt" << std::endl;
}

/* the chains the context has contracted (nc composite edges, nl links), as the host's partial simplification takes them */
static int fetch_chains(Job &J, disco_ctx *ctx, const char *ctx_name, uint64_t nc, uint64_t nl)
{
    J.ch_comp.resize(nc);
    J.ch_links.reset(new disco_chain_link[std::max<uint64_t>(nl, 1)]);
    J.ch_absorbed.reset(new uint8_t[J.e_out]);
    if (disco_fetch_chains(ctx, J.ch_comp.data(), J.ch_links.get(), J.ch_absorbed.get()) < 0)
        return die(std::string("disco_fetch_chains(") + ctx_name + ", ch_comp.data(), ch_links.get(), ch_absorbed.get()) : " + disco_last_error(ctx));
    return GO_ON;
}

/* ---- the device writes the files of one kind ----------------------------------------------------------------------------------------
 * format (or prepare) on the device — a soft error (DISCO_E_NOMEM / DISCO_E_UNSUPPORTED) hands the product to the host writer (demote) and
 * the run goes on — then open the files, write them through the ring, close them, print the lap. Every other error goes to `fail`: the
 * single-GPU path returns through die, a rank thread prints and _exit(2)s. The descriptors are closed whichever way this is left. */
struct DeviceFiles {
    disco::Product product;
    disco_ctx *ctx;
    std::string handed;                 /* verbose note when the host writer takes the product over */
    const char *lap_format, *lap_write; /* (null: no lap there) */
    const char *err_format = "", *err_write = ""; /* what `fail` hears in front of the library's message */
    bool soft_format = true, soft_write = false;  /* a soft error of that step demotes; otherwise it ends the run like any other */
};
using Lap = std::function<void(const char *)>;
using Fail = std::function<int(const std::string &)>;

template <class Format, class Formatted, class Open, class Write>
static int device_writes(bool verbose, disco::OutputPlan &plan, const DeviceFiles &d, const Lap &lap, const Fail &fail, Format format, Formatted formatted, Open open, Write write)
{
    auto soft = [](int64_t rc) { return rc == DISCO_E_NOMEM || rc == DISCO_E_UNSUPPORTED; };
    auto hand_over = [&]() {
        if (verbose) fprintf(stderr, "[disco host] %s: %s\n", d.handed.c_str(), disco_last_error(d.ctx));
        plan.demote(d.product);
        return GO_ON;
    };
    const int64_t n = format();
    if (n < 0) return d.soft_format && soft(n) ? hand_over() : fail(std::string(d.err_format) + disco_last_error(d.ctx));
    if (d.lap_format) lap(d.lap_format);
    formatted(n);
    Fds fds;
    std::string err;
    if (!open(n, fds, err)) return fail(err);
    const int rc = write(fds);
    fds.close_all();
    if (rc < 0) return d.soft_write && soft(rc) ? hand_over() : fail(std::string(d.err_write) + disco_last_error(d.ctx));
    if (d.lap_write) lap(d.lap_write);
    return GO_ON;
}

/* --par-simple on one GPU, the files from the device: contract -> residue, headers, first edges -> the host rounds on that small graph ->
 * the lines from the device's own link arrays into the open files (disco_format_par_simple): the edges, the links and the text never lie on
 * the host. A call that has no memory or does not support the case hands the run back to the flow through the host (write_host_outputs). */
static int par_simple_on_device(Job &J, disco_ctx *ctx, const Lap &lap, const Fail &fail, const std::function<bool()> &fetch_edges)
{
    const Args &a = J.a;
    disco::ReadSet &rs = J.rs;
    const uint32_t min_overlap_simplify = a.min_overlap_simplify;
    std::vector<disco_chain_edge> &ch_comp = J.ch_comp;
    const std::unique_ptr<uint16_t[]> &edge_file = J.edge_file;
    uint64_t nc = 0, nl = 0;
    DISCO_CALL(ctx, disco_contract_chains(ctx, min_overlap_simplify, &nc, &nl));
    const int n_ps_files = a.threads;
    auto soft = [](int64_t rc) { return rc == DISCO_E_NOMEM || rc == DISCO_E_UNSUPPORTED; };
    const int64_t nres = disco_fetch_chain_residue(ctx, nullptr, nullptr, 0);
    if (nres < 0) return die(disco_last_error(ctx));
    std::vector<uint64_t> res_index((size_t)nres), first_edge(nc);
    std::vector<disco_edge> res_edges((size_t)nres);
    ch_comp.resize(nc);
    int64_t rc = disco_fetch_chain_residue(ctx, res_index.data(), res_edges.data(), (uint64_t)nres);
    if (rc >= 0) rc = disco_fetch_chains(ctx, ch_comp.data(), nullptr, nullptr);
    if (rc >= 0) rc = disco_fetch_chain_first_edges(ctx, first_edge.data());
    std::vector<disco_chain_link> comp_first(nc), comp_last_rev(nc);
    if (rc >= 0) rc = disco_fetch_chain_end_links(ctx, comp_first.data(), comp_last_rev.data());
    if (soft(rc)) {
        if (J.verbose) fprintf(stderr, "[disco host] partial simplification through the host: %s: %s\n", "fetching the residue", disco_last_error(ctx));
        J.plan.demote(disco::PAR_SIMPLE);
    } else if (rc < 0)
        return die(disco_last_error(ctx));
    lap("contract chains on the GPU");
    if (J.plan.device(disco::PAR_SIMPLE)) {
        std::vector<uint16_t> res_file((size_t)nres), comp_file(nc);
        for (int64_t i = 0; i < nres; i++) res_file[(size_t)i] = edge_file[res_index[(size_t)i]];
        for (uint64_t k = 0; k < nc; k++) comp_file[k] = edge_file[first_edge[k]];
        disco::ChainResidue res;
        res.edges = res_edges.data();
        res.edge_file = res_file.data();
        res.n_edges = (uint64_t)nres;
        res.comp = ch_comp.data();
        res.comp_file = comp_file.data();
        res.n_comp = nc;
        res.comp_first = comp_first.data();
        res.comp_last_rev = comp_last_rev.data();
        disco::ParSimpleDescription desc;
        disco::ParSimpleStats ps;
        if (!disco::write_par_simple_residue(a.par_simple, n_ps_files, res, rs, J.err, &ps, nullptr, nullptr, &desc)) return die(J.err);
        lap("partial simplification: host rounds");
        std::vector<uint64_t> poff((size_t)n_ps_files + 1, 0);
        const DeviceFiles d{disco::PAR_SIMPLE, ctx, "partial simplification through the host: formatting the lines", nullptr, "partial simplification"};
        const int drc = device_writes(
            J.verbose, J.plan, d, lap, fail,
            [&]() {
                return disco_format_par_simple(ctx, (uint32_t)n_ps_files, J.ids(), desc.edges.data(), desc.edges.size(), desc.pieces.data(), desc.pieces.size(), poff.data());
            },
            [&](int64_t nb) {
                if (J.verbose)
                    fprintf(stderr, "[disco host] partial simplification on the GPU: residue %lld edges + %llu composite edges -> %zu final edges in %zu pieces (%llu reversed, at most %u in one edge), %lld bytes of text\n",
                            (long long)nres, (unsigned long long)nc, desc.edges.size(), desc.pieces.size(), (unsigned long long)desc.reversed_pieces, desc.max_pieces, (long long)nb);
            },
            [&](int64_t, Fds &fds, std::string &err) {
                const disco::FileTags pt = disco::FileTags::plain(a.threads);
                fds.fd.assign((size_t)n_ps_files, -1);
                for (int t = 0; t < n_ps_files; t++) {
                    const std::string path = a.par_simple + "_" + pt.tag[(size_t)t] + "_ParSimpleEdges.txt";
                    fds.fd[(size_t)t] = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
                    if (fds.fd[(size_t)t] < 0) {
                        err = "Unable to write file: " + path;
                        return false;
                    }
                }
                return true;
            },
            [&](Fds &fds) {
                const int wrc = disco_write_par_simple_text(ctx, fds.data(), (uint32_t)n_ps_files, (uint32_t)a.threads);
                if (wrc >= 0) print_par_simple_summary(J, ps); /* (closed right behind this; the summary stands in front of the lap) */
                return wrc;
            });
        if (drc != GO_ON) return drc;
    }
    if (!J.plan.device(disco::PAR_SIMPLE)) { /* handed back: what the flow through the host works on */
        if (!J.edges && !fetch_edges()) return die(disco_last_error(ctx));
        return fetch_chains(J, ctx, "ctx", nc, nl);
    }
    return GO_ON;
}

/* <prefix>.gfa (--gfa, --gfa-no-seq): the reduced graph as GFA 1.0, formatted on the GPU and sent through the pinned ring into the file
 * (disco_write_gfa). No product of the plan: the host has no maker for it, so every failure is an error of the run */
static int write_gfa_file(Job &J, disco_ctx *ctx)
{
    const std::string path = J.a.prefix + ".gfa";
    Fds fds;
    fds.fd.assign(1, open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666));
    if (fds.fd[0] < 0) return die("Unable to open file: " + path);
    const auto t = Clock::now();
    const int64_t nb = disco_write_gfa(ctx, fds.fd[0], J.ids(), J.a.gfa_no_seq ? DISCO_GFA_NO_SEQ : 0u, 0, (uint32_t)J.a.threads);
    if (nb < 0) return die(std::string("disco_write_gfa : ") + disco_last_error(ctx));
    const double s = secs(t);
    if (J.verbose) fprintf(stderr, "[disco host] GFA: %lld bytes in %.3f s (%.2f GB/s)\n", (long long)nb, s, s > 0 ? (double)nb / s * 1e-9 : 0.0);
    J.lap("GFA from the GPU into the file");
    return GO_ON;
}

/* <prefix>.unitigs.gfa (--gfa-unitigs): the compacted graph — every chain one segment with its merged bases (disco_write_gfa_chains). A
 * stage of its own behind every planned product and --gfa: it contracts for itself, every overlap counted (filter 0), whatever
 * --par-simple contracted before (its files are written, and what the host needs of that contraction it holds). No product of the plan */
static int write_gfa_unitigs_file(Job &J, disco_ctx *ctx, uint64_t &nc, uint64_t &nl)
{
    const std::string path = J.a.prefix + ".unitigs.gfa";
    auto t = Clock::now();
    DISCO_CALL(ctx, disco_contract_chains(ctx, 0, &nc, &nl));
    const double s_contract = secs(t);
    Fds fds;
    fds.fd.assign(1, open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666));
    if (fds.fd[0] < 0) return die("Unable to open file: " + path);
    t = Clock::now();
    const int64_t nb = disco_write_gfa_chains(ctx, fds.fd[0], J.ids(), J.a.gfa_no_seq ? DISCO_GFA_NO_SEQ : 0u, 0, (uint32_t)J.a.threads);
    if (nb < 0) return die(std::string("disco_write_gfa_chains : ") + disco_last_error(ctx));
    const double s = secs(t);
    if (J.verbose)
        fprintf(stderr, "[disco host] GFA of unitigs: %llu chains of %llu links contracted in %.3f s; %lld bytes in %.3f s (%.2f GB/s)\n", (unsigned long long)nc, (unsigned long long)nl,
                s_contract, (long long)nb, s, s > 0 ? (double)nb / s * 1e-9 : 0.0);
    J.lap("GFA of unitigs from the GPU into the file");
    return GO_ON;
}

/* <prefix>.unitigs.reads (--unitig-reads; --unitig-depth: its U lines only): every read placed on its segment of the compacted graph
 * (disco_write_unitig_reads). A stage of its own directly behind --gfa-unitigs', whose contraction it shares (contracted: nc, nl are
 * that one's); alone it contracts for itself, every overlap counted. No product of the plan: every failure is an error of the run */
static int write_unitig_reads_file(Job &J, disco_ctx *ctx, bool contracted, uint64_t nc, uint64_t nl)
{
    const std::string path = J.a.prefix + ".unitigs.reads";
    auto t = Clock::now();
    if (!contracted) DISCO_CALL(ctx, disco_contract_chains(ctx, 0, &nc, &nl));
    const double s_contract = secs(t);
    Fds fds;
    fds.fd.assign(1, open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666));
    if (fds.fd[0] < 0) return die("Unable to open file: " + path);
    t = Clock::now();
    const int64_t nb = disco_write_unitig_reads(ctx, fds.fd[0], J.ids(), J.a.unitig_reads ? 0u : DISCO_UNITIG_READS_DEPTH_ONLY, 0, (uint32_t)J.a.threads);
    if (nb < 0) return die(std::string("disco_write_unitig_reads : ") + disco_last_error(ctx));
    const double s = secs(t);
    if (J.verbose) /* (the rounds of doubling and the time of the kernels that resolve and count stand in the library's own line) */
        fprintf(stderr, "[disco host] reads on unitigs%s: %llu chains of %llu links %s in %.3f s; %lld bytes in %.3f s (%.2f GB/s)\n", J.a.unitig_reads ? "" : " (depth only)",
                (unsigned long long)nc, (unsigned long long)nl, contracted ? "shared with the GFA of unitigs" : "contracted", s_contract, (long long)nb, s, s > 0 ? (double)nb / s * 1e-9 : 0.0);
    J.lap("reads on unitigs from the GPU into the file");
    return GO_ON;
}

/* ---- the graph on one GPU, and every file the device writes ------------------------------------------------------------------------- */
static int graph_single_gpu(Job &J)
{
    const Args &a = J.a;
    disco::OutputPlan &plan = J.plan;
    disco::ReadSet &rs = J.rs;
    uint64_t &n_cont = J.n_cont, &e_pre = J.e_pre, &e_out = J.e_out;
    std::unique_ptr<uint16_t[]> &edge_file = J.edge_file;
    std::unique_ptr<char[]> &edge_text = J.edge_text;
    const uint32_t min_overlap_simplify = a.min_overlap_simplify, threads = (uint32_t)a.threads;
    const uint32_t n_edge_files = (uint32_t)plan.opt.n_edge_files, ncf = (uint32_t)J.ctags.tag.size();
    const disco_params prm = make_params(a);
    disco_ctx *ctx = J.ctx1;
    if (!ctx && disco_create(a.gpu, &prm, &ctx) < 0) return die(std::string("disco_create: ") + disco_last_error(nullptr));
    if (!J.ingested) DISCO_CALL(ctx, disco_upload_reads_ragged(ctx, rs.packed, rs.len.data(), rs.size()));
    J.t_h2d = secs(J.t0);
    J.t0 = Clock::now();
    DISCO_CALL(ctx, disco_build_index(ctx));
    DISCO_CALL(ctx, disco_probe(ctx));
    DISCO_CALL(ctx, disco_mark_contained(ctx, &n_cont));
    print_contained_counts(J);
    /* where the rows are wanted on the host (binary side output by the host writer, DISCO_HOST_TEXT / DISCO_HOST_CONTAINED_TEXT=1), they
     * leave now, grouped for their files, while the edges are selected and reduced */
    if (plan.rows_early && n_cont) (void)disco_start_contained_rows(ctx, 1);
    DISCO_CALL(ctx, disco_build_edges(ctx, &e_pre));
    DISCO_CALL(ctx, disco_transitive_reduce(ctx, &e_out));
    J.t_graph = secs(J.t0);
    disco_counters cn;
    DISCO_CALL(ctx, disco_get_counters(ctx, &cn));
    std::ostringstream fin;
    fin << "Function buildOverlapGraph() [GPU] finished in " << J.t_graph << " Seconds (" << (J.t_graph > 0 ? e_pre / J.t_graph : 0) << " overlaps/s); host->device " << J.t_h2d
        << " Seconds.";
    print_graph_summary(J, "", cn.probes, cn.kmer_hits, cn.cap_bind_sites, cn.asymmetric_pairs, "", fin.str());
    J.t0 = Clock::now();
    J.t1 = Clock::now();
    if (!J.join_ingest_fetch()) return die(disco_last_error(ctx));
    J.lap("wait for lengths + file indices");
    const Lap lap = [&J](const char *what) { J.lap(what); };
    const Fail fail = [](const std::string &msg) { return die(msg); };
    const auto nothing = [](int64_t) {};
    int rc = GO_ON;
    /* the contained-read files from the GPU (disco_format_contained: rows grouped, sorted and formatted where the keys are, the lines
     * through the pinned ring into the files), right behind the reduction: the ring is free, and nothing of the rows crosses to the host */
    if (plan.device(disco::CONTAINED_TEXT)) {
        std::vector<uint64_t> coff((size_t)ncf + 1, 0);
        rc = device_writes(
            J.verbose, plan, {disco::CONTAINED_TEXT, ctx, "contained lines by the host writer", "format contained lines on the GPU", "contained lines into the files"}, lap, fail,
            [&]() { return disco_format_contained(ctx, ncf, J.ids(), coff.data()); }, nothing,
            [&](int64_t, Fds &fds, std::string &err) {
                fds.fd.assign(ncf, -1);
                return disco::open_contained_files(a.prefix, (int)ncf, &J.ctags, fds.data(), err);
            },
            [&](Fds &fds) { return disco_write_contained_text(ctx, fds.data(), ncf, threads); });
        if (rc != GO_ON) return rc;
    }
    /* <prefix>_contained.bin / _edges.bin: the header from here, the records from the device (grouped and sorted there) into the open file */
    auto binary_records = [&](disco::Product product, bool contained, const char *kind, const std::function<int64_t()> &prepare, const std::function<int(int)> &write) {
        DeviceFiles d{product, ctx, std::string("binary ") + kind + " records by the host writer", nullptr, contained ? "binary contained records on the GPU" : "binary edge records on the GPU"};
        d.soft_write = true;
        return device_writes(
            J.verbose, plan, d, lap, fail, prepare, nothing,
            [&](int64_t nr, Fds &fds, std::string &err) {
                fds.fd.assign(1, disco::open_binary_records(a.prefix, contained, (uint64_t)nr, contained ? (int)ncf : (int)n_edge_files, err));
                return fds.fd[0] >= 0;
            },
            [&](Fds &fds) { return write(fds.fd[0]); });
    };
    if (plan.device(disco::CONTAINED_BIN)) {
        rc = binary_records(disco::CONTAINED_BIN, true, "contained", [&]() { return disco_prepare_contained_records(ctx, ncf, J.ids()); },
                            [&](int fd) { return disco_write_contained_records(ctx, fd, 32, threads); });
        if (rc != GO_ON) return rc;
    }
    if (plan.rows_on_host()) J.rows.resize(n_cont);
    if (n_cont && plan.rows_on_host()) { /* in the files' order where the device grouped them during the pass; by id (sorted by the writer) otherwise */
        const int64_t grc = plan.rows_grouped ? disco_fetch_contained_grouped(ctx, J.rows.data(), n_cont) : (int64_t)DISCO_E_UNSUPPORTED;
        J.rows_grouped = grc >= 0;
        if (grc < 0 && grc != DISCO_E_UNSUPPORTED) return die(disco_last_error(ctx));
        if (!J.rows_grouped && disco_fetch_contained(ctx, J.rows.data(), n_cont) < 0) return die(disco_last_error(ctx));
    }
    J.lap("fetch contained rows");
    /* the contained-read files are written by a thread of their own while the device partitions and formats the edges (their rows
     * have been final since the contained flags were fixed); joined before the checkpoint is written */
    if (plan.contained_by_writer_thread())
        J.contained_writer.t = std::thread([&J]() {
            std::string e2;
            J.contained_ok = disco::write_contained(J.a.prefix, (int)J.ctags.tag.size(), J.rows, J.rs, e2, &J.ctags, J.rows_grouped);
            if (!J.contained_ok) J.contained_err = e2;
        });
    /* connected components of the reduced graph dealt out to the files: every node has all its edges in one file, which is
     * what lets parsimplify work on the files independently (the reference gets it from its BFS batches) */
    edge_file.reset(new uint16_t[std::max<uint64_t>(e_out, 1)]);
    if (e_out && disco_fetch_edge_files(ctx, n_edge_files, edge_file.get(), e_out) < 0) return die(disco_last_error(ctx));
    J.lap("partition edges into files");
    /* the edge lines of the text files formatted where the edges are (2.5 GB of numbers at config 3), then straight from the device into the
     * edge files (pieces through a pinned ring, host threads pwrite behind the copies) or fetched for write_edge_text. EVERY error of
     * disco_format_edges ends the run. Without an edge there is nothing to format: the host writer creates the empty files */
    if (!e_out) plan.demote(disco::EDGE_TEXT);
    if (plan.device(disco::EDGE_TEXT)) {
        const bool stream = plan.stream_edge_text;
        uint64_t nb = 0;
        J.edge_text_off.assign((size_t)n_edge_files + 1, 0);
        DeviceFiles d{disco::EDGE_TEXT, ctx, "", "format edge lines on the GPU", stream ? "edge lines into the files" : "fetch edge lines"};
        d.soft_format = false;
        if (!stream) d.err_write = "disco_fetch_edge_text(ctx, edge_text.get(), (uint64_t)nb) : ";
        rc = device_writes(
            J.verbose, plan, d, lap, fail, [&]() { return disco_format_edges(ctx, n_edge_files, edge_file.get(), J.ids(), J.edge_text_off.data()); }, nothing,
            [&](int64_t n, Fds &fds, std::string &err) {
                nb = (uint64_t)n;
                if (!stream) edge_text.reset(new char[std::max<int64_t>(n, 1)]);
                if (stream) fds.fd.assign(n_edge_files, -1);
                return !stream || disco::open_edge_files(a.prefix, (int)n_edge_files, &J.etags, rs.size(), fds.data(), err);
            },
            [&](Fds &fds) { return stream ? disco_write_edge_text(ctx, fds.data(), n_edge_files, threads) : disco_fetch_edge_text(ctx, edge_text.get(), nb); });
        if (rc != GO_ON) return rc;
    }
    auto fetch_edges = [&]() -> bool {
        J.edges.reset(new disco_edge[std::max<uint64_t>(e_out, 1)]); /* 1.8 GB at 45 M edges: not zero-filled first */
        if (e_out && disco_fetch_edges(ctx, J.edges.get(), e_out) < 0) return false;
        if (a.max_subs) {
            J.edge_subs.reset(new uint16_t[std::max<uint64_t>(e_out, 1)]);
            if (e_out && disco_fetch_edge_substitutions(ctx, J.edge_subs.get(), e_out) < 0) return false;
        }
        J.lap("fetch edges");
        return true;
    };
    /* <prefix>_edges.bin from the device: any number of files, substitutions included (the edge TEXT of such runs stays with the host writer) */
    if (plan.device(disco::EDGES_BIN)) {
        rc = binary_records(disco::EDGES_BIN, false, "edge", [&]() { return disco_prepare_edge_records(ctx, n_edge_files, edge_file.get(), J.ids()); },
                            [&](int fd) { return disco_write_edge_records(ctx, fd, 32, threads); });
        if (rc != GO_ON) return rc;
    }
    if (plan.edges_on_host() && !fetch_edges()) return die(disco_last_error(ctx));
    if (!e_out) plan.demote(disco::PAR_SIMPLE); /* (no edge, no chain: the host writer creates the empty files) */
    if (plan.device(disco::PAR_SIMPLE)) rc = par_simple_on_device(J, ctx, lap, fail, fetch_edges);
    else if (plan.chains_on_device && e_out) {
        uint64_t nc = 0, nl = 0;
        DISCO_CALL(ctx, disco_contract_chains(ctx, min_overlap_simplify, &nc, &nl));
        rc = fetch_chains(J, ctx, "ctx", nc, nl);
        if (rc == GO_ON) J.lap("contract chains on the GPU");
    }
    if (rc != GO_ON) return rc;
    if (a.gfa && (rc = write_gfa_file(J, ctx)) != GO_ON) return rc;
    uint64_t u_nc = 0, u_nl = 0;
    if (a.gfa_unitigs && (rc = write_gfa_unitigs_file(J, ctx, u_nc, u_nl)) != GO_ON) return rc;
    if ((a.unitig_reads || a.unitig_depth) && (rc = write_unitig_reads_file(J, ctx, a.gfa_unitigs, u_nc, u_nl)) != GO_ON) return rc;
    /* the context is released by a thread of its own while the files are written (0.07 s of hipFree at config 3) */
    J.ctx_releaser.t = std::thread([ctx]() { disco_destroy(ctx); });
    J.lap("release GPU context (in the background)");
    return GO_ON;
}

struct RankResult {
    std::vector<disco_contained_row> rows;
    std::unique_ptr<disco_edge[]> edges;
    std::unique_ptr<uint16_t[]> subs; /* inexact mode only */
    uint64_t n_edges = 0;
    disco_dist_info info{};
    /* the rank's own copy of the plan: it wrote its share of the files from its GPU (disco_dist_format_contained / disco_dist_format_edges) or
     * demoted the product; the library makes the ranks agree, so the copies end alike on every rank */
    disco::OutputPlan plan;
    Clock::time_point pass_end{};
};

/* one rank of --gpus N: its reads up, the pass, its share of the files or of the records */
static void rank_thread(Job &J, int r, RankResult &R, const std::vector<uint64_t> &woff)
{
    const Args &a = J.a;
    disco::ReadSet &rs = J.rs;
    const int gpus = a.gpus;
    disco_ctx *c = J.ctx[(size_t)r];
    auto at = [&](int x) { J.stage[(size_t)r].store(x); };
    /* the other ranks wait for this one inside a collective: there is nothing to unwind to */
    const Fail fail = [r](const std::string &msg) -> int {
        std::cout << "\nError (rank " << r << "): " << msg << std::endl;
        _exit(2);
    };
    auto bail = [&](const char *what) { fail(std::string(what) + ": " + disco_last_error(c)); };
    if (!J.comm_joined) {
        at(ST_COMM_INIT);
        if (!a.same_device && disco_comm_init(c, J.uid, gpus, r) < 0) bail("disco_comm_init");
    }
    if (!J.ingested) { /* (the device input stage left the rank's home range in place, as the upload does) */
        uint64_t lo = 0, hi = 0;
        if (disco_dist_range(c, rs.size(), &lo, &hi) < 0) bail("disco_dist_range");
        at(ST_UPLOAD);
        const std::vector<uint64_t> own = rs.rows(lo, hi, woff); /* (the multi-GPU table has one stride: the rank's rows at it) */
        if (disco_dist_upload_reads(c, own.data(), rs.stride_words, rs.len.data() + lo, rs.size()) < 0) bail("disco_dist_upload_reads");
    }
    at(ST_FRONT_OF_PASS);
    /* (tests: a rank that never enters the pass; DISCO_TEST_STALL_FIRST_TRY: in the launcher's first child only) */
    if (getenv("DISCO_TEST_STALL_RANK") && atoi(getenv("DISCO_TEST_STALL_RANK")) == r &&
        (!getenv("DISCO_TEST_STALL_FIRST_TRY") || !getenv("DISCO_BUILDG_CHILD") || !strcmp(getenv("DISCO_BUILDG_CHILD"), "1")))
        for (;;) std::this_thread::sleep_for(std::chrono::seconds(1));
    at(ST_PASS);
    if (disco_dist_run_graph(c, DISCO_DIST_GATHER_READS | (a.partitioned_index ? DISCO_DIST_KEEP_INDEX_PARTITIONED : 0)) < 0) bail("disco_dist_run_graph");
    if (disco_dist_get_info(c, &R.info) < 0) bail("disco_dist_get_info");
    if (J.verbose && r == 0) fprintf(stderr, "[disco host] transport %s, %d ranks\n", disco_comm_kind(c), gpus);
    R.pass_end = Clock::now();
    /* The rank's share of the files from its GPU: the files f of a kind with floor(f gpus / files) == r. Both calls are collective
     * and end alike on every rank, so the ranks take the same way without asking each other: all of them write their files, or —
     * DISCO_E_UNSUPPORTED / DISCO_E_NOMEM — all of them hand their rows / edges to the host writer (write_host_outputs), in the same run */
    auto t_lap = Clock::now();
    const Lap rank_lap = [&](const char *what) {
        if (J.verbose) fprintf(stderr, "[disco host] rank %d: %-36s %.3f s\n", r, what, secs(t_lap));
        t_lap = Clock::now();
    };
    const std::string rank = "rank " + std::to_string(r) + ": ";
    const uint32_t threads = (uint32_t)a.threads;
    /* its files [lo, hi) of n_files of a kind, opened; the others' stay -1 */
    auto open_own = [&](int n_files, Fds &fds, std::string &err, bool edge_files) {
        const int lo = (int)(((int64_t)r * n_files + gpus - 1) / gpus), hi = (int)(((int64_t)(r + 1) * n_files + gpus - 1) / gpus);
        fds.fd.assign((size_t)n_files, -1);
        return edge_files ? disco::open_edge_files(a.prefix, n_files, &J.etags, rs.size(), fds.data(), err, lo, hi)
                          : disco::open_contained_files(a.prefix, n_files, &J.ctags, fds.data(), err, lo, hi);
    };
    if (R.plan.device(disco::CONTAINED_TEXT)) {
        at(ST_FORMAT_CONTAINED);
        const int ncf = (int)J.ctags.tag.size();
        std::vector<uint64_t> coff((size_t)ncf + 1, 0);
        DeviceFiles d{disco::CONTAINED_TEXT, c, rank + "contained lines by the host writer", "format contained lines on the GPU", "contained lines into the files",
                      "disco_dist_format_contained: ", "disco_write_contained_text: "};
        device_writes(
            J.verbose, R.plan, d, rank_lap, fail, [&]() { return disco_dist_format_contained(c, (uint32_t)ncf, J.ids(), coff.data()); }, [&](int64_t) { at(ST_WRITE_CONTAINED); },
            [&](int64_t, Fds &fds, std::string &err) { return open_own(ncf, fds, err, false); }, [&](Fds &fds) { return disco_write_contained_text(c, fds.data(), (uint32_t)ncf, threads); });
    }
    if (!R.plan.device(disco::CONTAINED_TEXT)) {
        at(ST_FETCH_CONTAINED);
        R.rows.resize(R.info.n_contained_local);
        if (R.info.n_contained_local && disco_fetch_contained(c, R.rows.data(), R.info.n_contained_local) < 0) bail("disco_fetch_contained");
    }
    if (R.plan.device(disco::EDGE_TEXT)) {
        at(ST_FORMAT_EDGES);
        const int n_edge_files = R.plan.opt.n_edge_files;
        std::vector<uint64_t> eoff((size_t)n_edge_files + 1, 0);
        DeviceFiles d{disco::EDGE_TEXT, c, rank + "edge lines by the host writer", "partition + format edge lines on the GPU", "edge lines into the files",
                      "disco_dist_format_edges: ", "disco_write_edge_text: "};
        device_writes(
            J.verbose, R.plan, d, rank_lap, fail, [&]() { return disco_dist_format_edges(c, (uint32_t)n_edge_files, J.ids(), eoff.data()); }, [&](int64_t) { at(ST_WRITE_EDGES); },
            [&](int64_t, Fds &fds, std::string &err) { return open_own(n_edge_files, fds, err, true); },
            [&](Fds &fds) { return disco_write_edge_text(c, fds.data(), (uint32_t)n_edge_files, threads); });
    }
    if (!R.plan.device(disco::EDGE_TEXT)) {
        at(ST_FETCH_EDGES);
        R.n_edges = R.info.e_out_local;
        R.edges.reset(new disco_edge[std::max<uint64_t>(R.n_edges, 1)]);
        if (R.n_edges && disco_fetch_edges(c, R.edges.get(), R.n_edges) < 0) bail("disco_fetch_edges");
        if (a.max_subs) {
            R.subs.reset(new uint16_t[std::max<uint64_t>(R.n_edges, 1)]);
            if (R.n_edges && disco_fetch_edge_substitutions(c, R.subs.get(), R.n_edges) < 0) bail("disco_fetch_edge_substitutions");
        }
    }
    at(ST_DONE);
}

/* ---- the graph on N ranks: one rank per GPU, one host thread per rank (replaces mpirun -np N of runDisco-MPI.sh:214-258): rank r holds the
 * reads [r*per, (r+1)*per), every exchange is an RCCL collective inside libdisco_hip.so -------------------------------------------------- */
static int graph_ranks(Job &J)
{
    const Args &a = J.a;
    disco::ReadSet &rs = J.rs;
    const int gpus = a.gpus;
    uint64_t &n_cont = J.n_cont, &e_pre = J.e_pre, &e_out = J.e_out;
    std::unique_ptr<disco_edge[]> &edges = J.edges;
    std::vector<disco_ctx *> &ctx = J.ctx;
    const uint32_t min_overlap_simplify = a.min_overlap_simplify;
    std::vector<RankResult> res((size_t)gpus);
    for (auto &R : res) R.plan = J.plan;
    const std::vector<uint64_t> woff = J.ingested ? std::vector<uint64_t>() : rs.word_offsets();
    if (ctx.empty())
        if (const std::string e = make_ranks(J); !e.empty()) return die(e);
    J.wd_paused.store(false);
    on_ranks(gpus, [&](int r) { rank_thread(J, r, res[(size_t)r], woff); });
    J.ranks_done.store(true);
    /* a demotion is collective: every rank's plan ends as rank 0's */
    for (auto &R : res)
        if (R.plan.maker[disco::CONTAINED_TEXT] != res[0].plan.maker[disco::CONTAINED_TEXT] || R.plan.maker[disco::EDGE_TEXT] != res[0].plan.maker[disco::EDGE_TEXT])
            return die("the ranks disagree about who writes the text files");
    J.plan = res[0].plan;
    const bool dev_contained = J.plan.device(disco::CONTAINED_TEXT), dev_edges = J.plan.device(disco::EDGE_TEXT);
    /* (where the ranks wrote files, the graph was complete when the last rank left the pass: what they did behind it is output stage) */
    auto t_pass_end = Clock::now();
    if (dev_contained || dev_edges) {
        t_pass_end = res[0].pass_end;
        for (auto &R : res) t_pass_end = std::max(t_pass_end, R.pass_end);
    }
    J.t_graph = std::chrono::duration<double>(t_pass_end - J.t0).count();
    const disco_dist_info &di = res[0].info;
    n_cont = di.n_contained;
    e_pre = di.e_pre;
    e_out = di.e_out;
    print_contained_counts(J);
    std::ostringstream where, fin;
    where << " on " << gpus << " ranks" << (a.same_device ? " (one device, in-process exchanges)" : " (RCCL)");
    fin << "Function buildOverlapGraph() [" << gpus << " GPU ranks] finished in " << J.t_graph << " Seconds incl. upload (" << (J.t_graph > 0 ? e_pre / J.t_graph : 0)
        << " overlaps/s); last pass " << di.ms_total * 1e-3 << " Seconds on rank 0.";
    print_graph_summary(J, where.str(), di.probes, di.kmer_hits, di.cap_bind_sites, di.asymmetric_pairs,
                        std::string("  regime                   : ") +
                            (di.regime == 0   ? "regular (neighbour rows on request)"
                             : di.regime == 2 ? "regular after completing the lists of the reads that dropped a hit across ranks"
                                              : "order-dependent (adjacency gathered)") +
                            "\n",
                        fin.str());
    J.t0 = dev_contained || dev_edges ? t_pass_end : Clock::now();
    J.t1 = Clock::now();
    if (J.verbose && (dev_contained || dev_edges)) fprintf(stderr, "[disco host] %-28s %.3f s\n", "text files by the ranks", secs(t_pass_end));
    /* the ranks' shares side by side: contained rows of rank r's reads, edges whose smaller endpoint rank r owns */
    uint64_t nr = 0, ne = 0;
    for (auto &R : res) {
        nr += R.rows.size();
        ne += R.n_edges;
    }
    if ((!dev_contained && nr != n_cont) || (!dev_edges && ne != e_out)) return die("the ranks' shares do not add up to the job's totals");
    J.rows.reserve(nr);
    for (auto &R : res) {
        J.rows.insert(J.rows.end(), R.rows.begin(), R.rows.end());
        std::vector<disco_contained_row>().swap(R.rows);
    }
    edges.reset(new disco_edge[std::max<uint64_t>(ne, 1)]);
    if (a.max_subs) J.edge_subs.reset(new uint16_t[std::max<uint64_t>(ne, 1)]);
    uint64_t at = 0;
    for (auto &R : res) {
        if (R.n_edges) memcpy(edges.get() + at, R.edges.get(), R.n_edges * sizeof(disco_edge));
        if (R.n_edges && a.max_subs) memcpy(J.edge_subs.get() + at, R.subs.get(), R.n_edges * sizeof(uint16_t));
        at += R.n_edges;
        R.edges.reset();
        R.subs.reset();
    }
    J.lap("gather the ranks' shares");
    if (!dev_edges) {
        J.edge_file.reset(new uint16_t[std::max<uint64_t>(e_out, 1)]);
        if (e_out && disco_partition_edges(ctx[0], edges.get(), e_out, rs.size(), (uint32_t)J.plan.opt.n_edge_files, J.edge_file.get()) < 0) return die(disco_last_error(ctx[0]));
        J.lap("partition edges into files");
    }
    if (J.plan.chains_on_device && e_out) { /* the ranks' edges lie on the host: rank 0's context, which holds every read's length, contracts them */
        uint64_t nc = 0, nl = 0;
        DISCO_CALL(ctx[0], disco_contract_chains_of(ctx[0], edges.get(), e_out, min_overlap_simplify, &nc, &nl));
        if (const int rc = fetch_chains(J, ctx[0], "ctx[0]", nc, nl); rc != GO_ON) return rc;
        J.lap("contract chains on the GPU");
    }
    for (auto c : ctx) disco_destroy(c);
    J.lap("release GPU contexts");
    return GO_ON;
}

/* ---- what the plan leaves to the host: its writers for every product that is not the device's, then the checkpoint ------------------- */
static int write_host_outputs(Job &J)
{
    const Args &a = J.a;
    const disco::OutputPlan &plan = J.plan;
    disco::ReadSet &rs = J.rs;
    std::string &err = J.err;
    const int nef = (int)J.etags.tag.size(), ncf = (int)J.ctags.tag.size();
    const uint16_t *edge_file = J.e_out ? J.edge_file.get() : nullptr;
    if (plan.host(disco::EDGES_BIN) || plan.host(disco::CONTAINED_BIN)) { /* (a file the device has written is left alone) */
        if (plan.host(disco::EDGES_BIN) && !disco::write_binary_edges(a.prefix, nef, J.edges.get(), J.e_out, edge_file, rs, err, J.edge_subs.get())) return die(err);
        if (plan.host(disco::CONTAINED_BIN) && !disco::write_binary_contained(a.prefix, ncf, J.rows, rs, err)) return die(err);
        J.lap("write binary side output");
    }
    if (plan.host(disco::PAR_SIMPLE)) {
        disco::ParSimpleStats ps;
        disco::ChainSeed seed;
        if (J.ch_absorbed) {
            seed.comp = J.ch_comp.data();
            seed.n_comp = J.ch_comp.size();
            seed.links = J.ch_links.get();
            seed.absorbed = J.ch_absorbed.get();
        }
        if (!disco::write_par_simple(a.par_simple, nef, J.edges.get(), J.e_out, edge_file, rs, a.min_overlap_simplify, a.threads, err, &ps, nullptr, nullptr, nullptr,
                                     J.ch_absorbed ? &seed : nullptr))
            return die(err);
        print_par_simple_summary(J, ps);
        J.lap("partial simplification");
    }
    if (a.no_text) { /* the file lists of the scripts still exist (the consumer aborts on a missing file), empty */
        J.rows.clear();
        J.e_out = 0;
    }
    if (plan.device(disco::CONTAINED_TEXT)) { /* written while the text left the device */
    } else if (J.contained_writer.t.joinable()) {
        J.contained_writer.t.join();
        if (!J.contained_ok) return die(J.contained_err);
    } else if (!disco::write_contained(a.prefix, ncf, J.rows, rs, err, &J.ctags, J.rows_grouped))
        return die(err);
    J.lap("write contained rows");
    if (!disco::write_checkpoint(a.prefix, true, false, false, err)) return die(err);
    if (plan.edge_text_streamed()) { /* written while the text left the device */
    } else if (J.edge_text && !a.no_text) {
        if (!disco::write_edge_text(a.prefix, nef, J.edge_text.get(), J.edge_text_off.data(), rs.size(), err, &J.etags)) return die(err);
    } else if (!disco::write_edges(a.prefix, nef, J.edges.get(), J.e_out, rs, a.threads, err, J.e_out ? J.edge_file.get() : nullptr, &J.etags, J.edge_subs.get()))
        return die(err);
    J.lap("write edges");
    if (!disco::write_checkpoint(a.prefix, false, true, true, err)) return die(err);
    return GO_ON;
}

/* Every file is written and closed, the checkpoint says so: the stage is over. What is left is tearing down the GPU runtime — tens of
 * GB of device memory, its streams and events, the libraries' static state: 0.15-0.2 s at config 3 that produce nothing (the
 * driver takes everything back when the process ends, whichever way it ends). DISCO_ORDERLY_EXIT=1 keeps the long way (leak
 * checkers, tests that want the destructors to run). */
/* round 6: the orderly way is the DEFAULT whenever somebody may be listening at exit — a profiler or tracer preloaded into the
 * process (rocprofv3 / roctx write their output from atexit handlers and tool finalizers: `rocprofv3 --marker-trace -- buildG ...` of
 * DESIGN.md section 1 lost its trace to the quick exit), LD_PRELOAD in general, coverage and sanitizer runtimes, DISCO_TRACE.
 * DISCO_QUICK_EXIT=1 forces the short way, DISCO_ORDERLY_EXIT=1 the long one. */
static int leave(Job &J)
{
    const bool tool_attached = getenv("ROCP_TOOL_LIBRARIES") || getenv("ROCPROFILER_REGISTER_FORCE_LOAD") || getenv("HSA_TOOLS_LIB") || getenv("LD_PRELOAD") ||
                               getenv("DISCO_TRACE") || getenv("GCOV_PREFIX") || getenv("ASAN_OPTIONS") || getenv("TSAN_OPTIONS") || getenv("UBSAN_OPTIONS");
    const bool orderly = getenv("DISCO_ORDERLY_EXIT") != nullptr || (tool_attached && !getenv("DISCO_QUICK_EXIT"));
    std::cout << "Function saveParGraphToFile() finished in " << secs(J.t0) << " Seconds." << std::endl;
    std::cout << "Function main() finished in " << secs(J.t_main) << " Seconds." << std::endl;
    /* PROPERTY 2: the releaser thread is JOINED before either way out of the process — leaving through _exit while it sits inside
     * disco_destroy / hipFree raced the runtime's own teardown (0.07 s of hipFree at config 3, nearly all of it behind the writers by now) */
    if (J.ctx_releaser.t.joinable()) J.ctx_releaser.t.join();
    if (!orderly) {
        std::cout.flush();
        std::cerr.flush();
        fflush(nullptr);
        _exit(0);
    }
    return 0;
}

int main(int argc, char **argv)
{
    auto t_main = Clock::now();
    setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0", 0); /* hosts with dmabuf IPC only: RCCL's buffer sharing needs it; before any HIP call */
    int launcher_gpus = 1; /* (a first look at the arguments for --gpus only; the real parse, with its messages, is the child's) */
    for (int i = 1; i + 1 < argc; i++)
        if (!strcmp(argv[i], "--gpus")) launcher_gpus = atoi(argv[i + 1]);
    /* ---- buildG --gpus N: a launcher that never touches the GPU, and the stage as its child (round 6) --------------------------------
     * Matches the role of mpirun in front of buildG-MPI (MPI/main.cpp:29-37; runDisco-MPI.sh:214-258): the process the user started owns
     * no device state, so it can start the stage again. When the stage's watchdog ends it (exit 3: no rank moved for DISCO_WATCHDOG_S
     * seconds — on first contact with a node that most likely means the two communicators of a context did not progress side by side),
     * the launcher starts ONE fresh child with DISCO_DIST_ONE_COMM=1 (every exchange on one communicator, one stream: the conservative
     * mode) before giving up. Never a re-exec of a process that has initialised the GPU; nothing was written that a second try could
     * trip over (the files appear after the pass, the checkpoint's GC=Complete line last). DISCO_NO_RETRY=1: one try only. */
    if (launcher_gpus > 1 && !getenv("DISCO_BUILDG_CHILD")) { /* (nothing printed yet: the child prints the stage's whole log, once) */
        std::cout.flush();
        auto run_child = [&](const char *attempt, bool one_comm) -> int {
            const pid_t pid = fork(); /* (single-threaded up to here: no thread pool, no GPU runtime thread) */
            if (pid < 0) return -1;
            if (pid == 0) {
                prctl(PR_SET_PDEATHSIG, SIGTERM); /* the stage does not outlive its launcher */
                setenv("DISCO_BUILDG_CHILD", attempt, 1);
                if (one_comm) setenv("DISCO_DIST_ONE_COMM", "1", 1);
                execv("/proc/self/exe", argv);
                perror("buildG: execv");
                _exit(127);
            }
            int st = 0;
            while (waitpid(pid, &st, 0) < 0 && errno == EINTR) {
            }
            return WIFEXITED(st) ? WEXITSTATUS(st) : 128 + (WIFSIGNALED(st) ? WTERMSIG(st) : 0);
        };
        int rc = run_child("1", false);
        if (rc == 3 && !getenv("DISCO_NO_RETRY") && !getenv("DISCO_DIST_ONE_COMM")) {
            std::cout << "\nThe multi-GPU stage made no progress and was ended by its watchdog; starting it ONCE more with one communicator "
                         "(DISCO_DIST_ONE_COMM=1)." << std::endl;
            rc = run_child("2", true);
        }
        if (rc < 0) {
            std::cerr << "buildG: fork failed" << std::endl;
            return 1;
        }
        return rc;
    }
    std::cout << "Software: Disco Assembler BuildGraph, MI355X-native drop-in (disco_amd)\n";
    if (disco_abi_version() != DISCO_ABI_VERSION) { /* the struct layouts this file was compiled against are those of exactly one version */
        std::cerr << "buildG: libdisco_hip.so speaks ABI version " << disco_abi_version() << ", this executable was built against " << DISCO_ABI_VERSION
                  << " (include/disco_hip.h): rebuild both (python -m disco_amd.build)" << std::endl;
        return 2;
    }
    Job J;
    J.t_main = t_main;
    Args &a = J.a;
    int rc = parse_args(argc, argv, a);
    if (rc != GO_ON) return rc;
    J.knobs = disco::read_knobs();
    J.verbose = getenv("DISCO_VERBOSE") != nullptr;
    J.stage = std::vector<std::atomic<int>>((size_t)a.gpus);
    for (auto &st : J.stage) st.store(ST_START);
    if ((rc = input_stage(J)) != GO_ON) return rc;
    if (a.par_simple.empty() && J.knobs.par_simple_env) par_simple_prefix_from_layout(a);
    /* who writes which file: decided here, once (output_plan.h); the stages ask the plan and demote in it */
    disco::Options opt;
    opt.gpus = a.gpus;
    opt.threads = a.threads;
    opt.no_text = a.no_text;
    opt.binary_out = a.binary_out;
    opt.par_simple = !a.par_simple.empty();
    opt.mpi_names = a.mpi_names;
    opt.max_subs = a.max_subs > 0;
    opt.count_files();
    J.plan = disco::plan(opt, J.knobs);
    J.etags = a.mpi_names ? disco::FileTags::mpi_edges(a.gpus, a.threads) : disco::FileTags::plain(a.threads);
    J.ctags = a.mpi_names ? disco::FileTags::mpi_contained(a.gpus, a.threads) : disco::FileTags::plain(a.threads);
    J.t0 = J.t1 = Clock::now();
    if ((rc = a.gpus == 1 ? graph_single_gpu(J) : graph_ranks(J)) != GO_ON) return rc;
    if ((rc = write_host_outputs(J)) != GO_ON) return rc;
    return leave(J);
}
