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
              << "  --no-text\tbinary output only: leave the text edge / contained files empty (a consumer with the loader patch)\n";
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

static int die(const std::string &msg)
{
    std::cout << "\nError: " << msg << std::endl; /* the reference prints and exits 0 (BG/Common.h:64); we exit non-zero */
    return 2;
}

#define DISCO_CALL(ctx, expr)                                                              \
    do {                                                                                   \
        if ((expr) < 0) return die(std::string(#expr " : ") + disco_last_error(ctx));      \
    } while (0)

struct RankResult {
    std::vector<disco_contained_row> rows;
    std::unique_ptr<disco_edge[]> edges;
    std::unique_ptr<uint16_t[]> subs; /* inexact mode only */
    uint64_t n_edges = 0;
    disco_dist_info info{};
    std::string err;
    /* the rank wrote its share of the files from its GPU (disco_dist_format_contained / disco_dist_format_edges): the library makes
     * the ranks agree, so these are the same on every rank */
    bool dev_contained = false, dev_edges = false;
    Clock::time_point pass_end{};
};

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
    std::vector<std::string> pe, se;
    std::string prefix, cfg;
    int threads = omp_get_max_threads(), gpu = 0, gpus = 1;
    bool same_device = false, mpi_names = false, binary_out = false, no_text = false, partitioned_index = false;
    std::string par_simple; /* prefix of the <prefix>_<i>_ParSimpleEdges.txt files, or empty */
    long long max_subs_cli = -1; /* --max-substitutions (overrides MaxSubstitutions4BuildGraph of the parameter file) */
    std::cout << "PRINTING ARGUMENTS\n";
    for (int i = 0; i < argc; i++) std::cout << argv[i] << ' ';
    std::cout << std::endl;
    if (argc == 1) {
        usage();
        return 0; /* BG/main.cpp:93-102 */
    }
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
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
                std::cerr << "Option " << a << " needs a number in [" << lo << ", " << hi << "]" << (t.empty() ? "" : ", got '" + t + "'") << "\n";
            }
            return v;
        };
        if (a == "-pe") for (auto &f : split(next(), ',')) pe.push_back(f);
        else if (a == "-se") for (auto &f : split(next(), ',')) se.push_back(f);
        else if (a == "-f") prefix = next();
        else if (a == "-t") threads = (int)num(1, 65534); /* one partial graph file per thread: 16-bit file index */
        else if (a == "-w") (void)num(0, ~0ull);
        else if (a == "-m") (void)num(0, ~0ull);
        else if (a == "-p") cfg = next();
        else if (a == "--gpu") gpu = (int)num(0, 1023);
        else if (a == "--gpus") gpus = (int)num(1, 64);
        else if (a == "--same-device") same_device = true;
        else if (a == "--partitioned-index") partitioned_index = true;
        else if (a == "--mpi-names") mpi_names = true;
        else if (a == "--par-simple") par_simple = next();
        else if (a == "--max-substitutions") max_subs_cli = (long long)num(0, 32767);
        else if (a == "--binary-out") binary_out = true;
        else if (a == "--no-text") binary_out = no_text = true;
        else {
            usage();
            if (a == "-h" || a == "--help") return 0;
            std::cerr << "Unknown option: " << a << "\n\n";
            return 1; /* BG/main.cpp:133-148 */
        }
        if (bad) {
            usage();
            return 1;
        }
    }
    uint32_t min_overlap = 30, min_overlap_simplify = 0, max_subs = 0;
    std::string cfg_err;
    if (!read_min_overlap(cfg, min_overlap, cfg_err, &min_overlap_simplify, &max_subs)) {
        std::cerr << "Unable to open parameter file: " << cfg << std::endl;
        return 1; /* BG/main.cpp:157-160 */
    }
    if (!cfg_err.empty()) {
        std::cerr << cfg_err << std::endl;
        return 1;
    }
    std::cout << "MinOverlap4BuildGraph = " << min_overlap << std::endl;
    disco::set_writer_threads(threads);
    if (max_subs_cli >= 0) max_subs = (uint32_t)max_subs_cli;
    if (max_subs)
        std::cout << "MaxSubstitutions4BuildGraph = " << max_subs << " (extension: overlaps and containments may differ in that many bases around an exact "
                  << "end-k-mer seed; the reference compares exactly)" << std::endl;

    bool ccr = false, gc = false;
    disco::read_checkpoint(prefix, ccr, gc);
    if (gc) { /* BG/main.cpp:48-52 */
        std::cout << "Graph already exists. Using previously built graph...\nExiting graph construction." << std::endl;
        return 0;
    }

    /* ---- reads -------------------------------------------------------------------------------------------------- */
    auto t0 = Clock::now();
    disco::ReadSet rs;
    std::string err;
    /* the packed reads go into ordinary memory: pinning 2 GB (hipHostMalloc) takes 0.5 s, which the upload then wins back only
     * 0.09 s of (0.09 against 0.18 s at config 3); DISCO_PINNED_READS=1 pins them all the same */
    disco::HostAlloc pinned;
    if (getenv("DISCO_PINNED_READS")) {
        pinned.alloc = disco_host_alloc;
        pinned.free = disco_host_free;
    }
    /* The input stage on the GPU (disco_ingest_fasta: the files travel to HBM as text; records, read filter, ids and the 2-bit rows are
     * kernels) for one GPU and plain FASTA / FASTQ files of the common form; DISCO_E_UNSUPPORTED (.gz, a '>' inside a line of a FASTA
     * file, irregularly wrapped long records, unreadable or empty files) leaves everything to the host stage below, which follows the reference's getline calls
     * literally and prints its messages. DISCO_HOST_INPUT=1: the host stage always. */
    disco_ctx *ctx1 = nullptr; /* the single-GPU context, created here when the device stage is tried */
    bool ingested = false;
    struct Joiner { /* (an early return must not leave a joinable thread behind) */
        std::thread t;
        ~Joiner()
        {
            if (t.joinable()) t.join();
        }
    } ingest_fetch_holder;
    std::thread &ingest_fetch = ingest_fetch_holder.t;
    std::atomic<int> ingest_fetch_rc{0};
    auto join_ingest_fetch = [&]() -> bool {
        if (ingest_fetch.joinable()) ingest_fetch.join();
        return ingest_fetch_rc.load() >= 0;
    };
    if (gpus == 1 && !getenv("DISCO_HOST_INPUT")) {
        const disco_params prm0{min_overlap, 4, DISCO_FLAG_SEEDED_KMER | (getenv("DISCO_EXACT_COUNTERS") ? 0u : DISCO_FLAG_TWO_PASS_VERIFY), max_subs};
        if (disco_create(gpu, &prm0, &ctx1) < 0) return die(std::string("disco_create: ") + disco_last_error(nullptr));
        if (getenv("DISCO_VERBOSE")) fprintf(stderr, "[disco host] process start to context ready   %.3f s\n", secs(t_main));
        std::vector<const char *> paths;
        for (auto &f : pe) paths.push_back(f.c_str());
        for (auto &f : se) paths.push_back(f.c_str());
        std::vector<disco_ingest_file> ifiles(paths.size());
        disco_ingest_info ii;
        const int irc = disco_ingest_fasta(ctx1, paths.data(), (int)paths.size(), (uint32_t)threads, &ii, ifiles.data());
        if (irc == DISCO_OK) {
            rs.n_reads = ii.n_reads;
            rs.stride_words = ii.stride_words;
            rs.total_records = ii.total_records;
            rs.too_long = ii.too_long;
            rs.shortest = ii.shortest;
            rs.longest = ii.longest;
            /* lengths and file indices of the reads come to the host on a thread of their own while the graph is built: only the
             * writers need them */
            ingest_fetch = std::thread([&rs, &ingest_fetch_rc, ctx1, n = ii.n_reads]() {
                const auto tf = Clock::now();
                /* (first touch by two threads: value-initialising 500 MB in one took 0.12 s, which the graph pass does not cover) */
                std::thread zl([&rs, n]() { rs.len.resize(n); });
                rs.file_index.resize(n);
                zl.join();
                const double tz = secs(tf);
                ingest_fetch_rc = disco_ingest_fetch(ctx1, rs.len.data(), rs.file_index.data());
                if (getenv("DISCO_VERBOSE")) fprintf(stderr, "[disco host] lengths + file indices to the host  %.3f s (of which first touch %.3f)\n", secs(tf), tz);
            });
            for (size_t i = 0; i < paths.size(); i++) {
                disco::FileRange fr;
                fr.name = paths[i];
                fr.paired = i < pe.size();
                fr.first_index = ifiles[i].first_index;
                fr.last_index = ifiles[i].last_index;
                fr.good = ifiles[i].good;
                fr.bad = ifiles[i].bad;
                rs.files.push_back(fr);
            }
            ingested = true;
            if (getenv("DISCO_VERBOSE"))
                fprintf(stderr, "[disco host] input stage on the GPU: files into HBM %.3f s, records + filter + ids + rows %.3f s\n", ii.read_s, ii.device_s);
        } else if (irc != DISCO_E_UNSUPPORTED)
            return die(std::string("disco_ingest_fasta: ") + disco_last_error(ctx1));
        else if (getenv("DISCO_VERBOSE"))
            fprintf(stderr, "[disco host] %s\n", disco_last_error(ctx1));
    }
    /* --gpus N: the contexts, the communicator and the watchdog exist BEFORE the input stage, because every rank reads its share of the
     * files itself (disco_dist_ingest_fasta: the bytes of the files laid end to end, cut into N shares; records, filter and rows on the
     * rank's GPU, rows of other ranks' home ranges sent to their owners). DISCO_E_UNSUPPORTED — on every rank alike: a .gz name (BGZF too, unless DISCO_DIST_BGZF=1 asks the ranks to decode it), a '>'
     * inside a line, an irregularly wrapped long record, an unreadable file — leaves the job to the host stage below, inside the same
     * run and on the same contexts. Asked for with DISCO_DIST_DEVICE_INPUT=1 (below: why not by default); DISCO_HOST_INPUT=1: the host stage always. */
    std::vector<disco_ctx *> ctx;
    unsigned char uid[DISCO_UNIQUE_ID_BYTES];
    bool comm_joined = false; /* (RCCL: the ranks joined the communicator in front of the device input stage) */
    /* Watchdog of the multi-rank stage (bench.py has its twin): every rank thread names the call it is in; when NO rank has moved for
     * DISCO_WATCHDOG_S seconds (default 900; 0: off) — a collective one rank never entered, a link that went away — the process says
     * where every rank stands and exits non-zero. Never a re-exec, never a silent hang: runDisco.sh does not check the status, but
     * the missing GC=Complete line makes the next run start over. */
    enum { ST_START = 0, ST_COMM_INIT, ST_INGEST, ST_INGEST_FETCH, ST_HOST_INPUT, ST_UPLOAD, ST_FRONT_OF_PASS, ST_PASS, ST_FETCH_CONTAINED, ST_FETCH_EDGES, ST_FORMAT_CONTAINED, ST_WRITE_CONTAINED, ST_FORMAT_EDGES, ST_WRITE_EDGES, ST_DONE };
    static const char *const kStage[] = {"start", "disco_comm_init", "disco_dist_ingest_fasta", "disco_dist_ingest_fetch", "the host input stage (between the rank threads)",
                                         "disco_dist_upload_reads", "front of disco_dist_run_graph (never entered it)", "disco_dist_run_graph",
                                         "disco_fetch_contained", "disco_fetch_edges", "disco_dist_format_contained", "disco_write_contained_text (its contained-read files)",
                                         "disco_dist_format_edges", "disco_write_edge_text (its edge files)", "done"};
    std::vector<std::atomic<int>> stage((size_t)gpus);
    for (auto &st : stage) st.store(ST_START);
    std::atomic<bool> ranks_done{false};
    const long wd_s = getenv("DISCO_WATCHDOG_S") ? atol(getenv("DISCO_WATCHDOG_S")) : 900;
    std::atomic<bool> wd_paused{false}; /* the host stage runs on the main thread: no rank moves, and nobody waits for one */
    std::thread watchdog;
    struct WatchdogJoin {
        std::atomic<bool> &done;
        std::thread &t;
        ~WatchdogJoin()
        {
            done.store(true);
            if (t.joinable()) t.join();
        }
    } watchdog_join{ranks_done, watchdog};
    /* the ranks' contexts, the communicator (in-process: joined here; RCCL: its id) and the watchdog; "" or what went wrong */
    auto make_ranks = [&]() -> std::string {
        const disco_params prm0{min_overlap, 4, DISCO_FLAG_SEEDED_KMER | (getenv("DISCO_EXACT_COUNTERS") ? 0u : DISCO_FLAG_TWO_PASS_VERIFY), max_subs};
        ctx.assign((size_t)gpus, nullptr);
        for (int r = 0; r < gpus; r++)
            if (disco_create(same_device ? gpu : gpu + r, &prm0, &ctx[(size_t)r]) < 0)
                return std::string("disco_create (rank ") + std::to_string(r) + "): " + disco_last_error(nullptr) +
                       (same_device ? "" : " — one GPU per rank is needed; --same-device runs all ranks on one GPU");
        if (same_device) {
            if (disco_comm_init_local(ctx.data(), gpus) < 0) return "disco_comm_init_local failed";
        } else if (disco_comm_unique_id(uid, sizeof uid) < 0)
            return std::string("disco_comm_unique_id: ") + disco_last_error(nullptr);
        watchdog = std::thread([&]() {
            if (wd_s <= 0) return;
            std::vector<int> last((size_t)gpus, -1);
            auto moved_at = Clock::now();
            while (!ranks_done.load()) {
                std::this_thread::sleep_for(std::chrono::milliseconds(200));
                bool moved = wd_paused.load();
                for (int r = 0; r < gpus; r++) {
                    const int x = stage[(size_t)r].load();
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
    };
    /* Measured (profiles/dist_ingest.txt): four ranks on ONE device, 5 M reads — the device stage on the ranks is not faster than the host
     * stage there (the ranks share one GPU and one link), so the host stage stays the default under --gpus N and
     * DISCO_DIST_DEVICE_INPUT=1 asks for the device stage; what one GPU per rank gains is a measurement this pool cannot make. */
    const char *ddi = getenv("DISCO_DIST_DEVICE_INPUT");
    if (gpus > 1 && ddi && strcmp(ddi, "0") != 0 && !getenv("DISCO_HOST_INPUT")) {
        if (const std::string e = make_ranks(); !e.empty()) return die(e);
        std::vector<const char *> paths;
        for (auto &f : pe) paths.push_back(f.c_str());
        for (auto &f : se) paths.push_back(f.c_str());
        /* reader threads per rank: all ranks together stay within 16 (one GPU: six keep the ring full, buildg's host has 16 cores). The
         * right figure for N links is a measurement nobody can make on this pool (its ranks share one device and one link). */
        const uint32_t readers = (uint32_t)std::max(1, std::min(threads, 16) / gpus);
        std::vector<int> irc((size_t)gpus, 0);
        std::vector<disco_dist_ingest_info> dii((size_t)gpus);
        std::vector<std::vector<disco_ingest_file>> ifiles((size_t)gpus, std::vector<disco_ingest_file>(paths.size()));
        auto on_ranks = [&](const std::function<void(int)> &fn) {
            std::vector<std::thread> th;
            for (int r = 0; r < gpus; r++) th.emplace_back(fn, r);
            for (auto &t : th) t.join();
        };
        on_ranks([&](int r) {
            disco_ctx *c = ctx[(size_t)r];
            stage[(size_t)r].store(ST_COMM_INIT);
            if (!same_device && disco_comm_init(c, uid, gpus, r) < 0) {
                /* the other ranks wait for this one inside a collective: there is nothing to unwind to */
                std::cout << "\nError (rank " << r << "): disco_comm_init: " << disco_last_error(c) << std::endl;
                _exit(2);
            }
            stage[(size_t)r].store(ST_INGEST);
            irc[(size_t)r] = disco_dist_ingest_fasta(c, paths.data(), (int)paths.size(), readers, &dii[(size_t)r], ifiles[(size_t)r].data());
        });
        comm_joined = true;
        bool all_ok = true, all_declined = true;
        for (int r = 0; r < gpus; r++) {
            all_ok = all_ok && irc[(size_t)r] == DISCO_OK;
            all_declined = all_declined && irc[(size_t)r] == DISCO_E_UNSUPPORTED;
        }
        if (all_ok) {
            const disco_dist_ingest_info &ii = dii[0];
            rs.n_reads = ii.n_reads;
            rs.stride_words = ii.stride_words;
            rs.total_records = ii.total_records;
            rs.too_long = ii.too_long;
            rs.shortest = ii.shortest;
            rs.longest = ii.longest;
            rs.len.resize(ii.n_reads);
            rs.file_index.resize(ii.n_reads);
            /* the ranks' home ranges, one behind the other, are the job's reads: lengths and file indices for _ReadIDMap.txt and the writers */
            on_ranks([&](int r) {
                stage[(size_t)r].store(ST_INGEST_FETCH);
                const disco_dist_ingest_info &d = dii[(size_t)r];
                if (d.home_hi > d.home_lo) irc[(size_t)r] = disco_dist_ingest_fetch(ctx[(size_t)r], rs.len.data() + d.home_lo, rs.file_index.data() + d.home_lo);
            });
            for (int r = 0; r < gpus; r++)
                if (irc[(size_t)r] < 0) return die(std::string("disco_dist_ingest_fetch: ") + disco_last_error(ctx[(size_t)r]));
            for (size_t i = 0; i < paths.size(); i++) {
                disco::FileRange fr;
                fr.name = paths[i];
                fr.paired = i < pe.size();
                fr.first_index = ifiles[0][i].first_index;
                fr.last_index = ifiles[0][i].last_index;
                fr.good = ifiles[0][i].good;
                fr.bad = ifiles[0][i].bad;
                rs.files.push_back(fr);
            }
            ingested = true;
            if (getenv("DISCO_VERBOSE"))
                for (int r = 0; r < gpus; r++)
                    fprintf(stderr, "[disco host] input stage on the GPU of rank %d: its bytes into HBM %.3f s, records + filter + ids + rows + exchange %.3f s\n", r, dii[(size_t)r].read_s,
                            dii[(size_t)r].device_s);
        } else if (!all_declined) {
            for (int r = 0; r < gpus; r++)
                if (irc[(size_t)r] != DISCO_OK && irc[(size_t)r] != DISCO_E_UNSUPPORTED) return die(std::string("disco_dist_ingest_fasta (rank ") + std::to_string(r) + "): " + disco_last_error(ctx[(size_t)r]));
            return die("disco_dist_ingest_fasta: the ranks disagree about the input");
        } else if (getenv("DISCO_VERBOSE"))
            fprintf(stderr, "[disco host] %s\n", disco_last_error(ctx[0]));
        for (auto &st : stage) st.store(ST_HOST_INPUT);
    }
    wd_paused.store(true);
    if (!ingested && !disco::load_reads(pe, se, min_overlap, threads, rs, err, pinned)) return die(err);
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
    if (!disco::write_read_id_map(prefix, rs, err)) return die(err);
    const double t_parse = secs(t0);
    std::cout << "Function readDataset() finished in " << t_parse << " Seconds." << std::endl;

    if (par_simple.empty() && getenv("DISCO_PAR_SIMPLE")) { /* runDisco.sh:166-167: <out>/graph/<name> and <out>/assembly/<name> */
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
            par_simple = base + "assembly/" + name;
            (void)mkdir((base + "assembly").c_str(), 0777); /* runDisco.sh keeps an existing assembly directory ("Will continue previous run") */
        } else
            std::cout << "DISCO_PAR_SIMPLE: the output prefix is not <out>/graph/<name>; use --par-simple <prefix>" << std::endl;
    }
    /* chains of the reduced graph contracted while it is still on the GPU (the consumer's parsimplify step, --par-simple) */
    const bool gpu_chains = !par_simple.empty() && !mpi_names && !getenv("DISCO_PAR_SIMPLE_HOST");
    /* ... and, on one GPU, its files written from there too: the host pass gets the residue of the contraction and the composite edges'
     * headers, describes every final line as pieces, and the device formats the lines from its own link arrays into the open files
     * (disco_format_par_simple) — the edges, the links and the text never lie on the host. DISCO_PAR_SIMPLE_GPU_TEXT=1 / =0 choose,
     * DISCO_PAR_SIMPLE_HOST_TEXT=1 forces the flow through the host (PAR_SIMPLE_GPU_TEXT_DEFAULT above says which is the default) */
    const char *psgt = getenv("DISCO_PAR_SIMPLE_GPU_TEXT");
    bool par_simple_on_gpu = gpu_chains && gpus == 1 && !max_subs && !getenv("DISCO_PAR_SIMPLE_HOST_TEXT") &&
                             (psgt ? strcmp(psgt, "0") != 0 : PAR_SIMPLE_GPU_TEXT_DEFAULT);
    bool par_simple_done = false;
    /* ... and the binary side output (GPU_BINARY_NO_TEXT_DEFAULT above): parsed as DISCO_DIST_GPU_TEXT is — 0 is off, anything else on */
    const char *gbin = getenv("DISCO_GPU_BINARY");
    const bool gpu_binary = binary_out && gpus == 1 && (gbin ? strcmp(gbin, "0") != 0 : (no_text && GPU_BINARY_NO_TEXT_DEFAULT));
    bool bin_contained_on_gpu = false, bin_edges_on_gpu = false; /* that file has been written from the device */
    std::unique_ptr<char[]> edge_text;     /* the edge lines, formatted on the GPU (single GPU, exact overlaps) */
    std::vector<uint64_t> edge_text_off;
    std::vector<disco_chain_edge> ch_comp;
    std::unique_ptr<disco_chain_link[]> ch_links;
    std::unique_ptr<uint8_t[]> ch_absorbed;
    /* ---- graph on the GPU(s) ---------------------------------------------------------------------------------------- */
    const bool verbose = getenv("DISCO_VERBOSE") != nullptr;
    /* two-pass verify for read sets of mixed lengths (metagenomes: most reads contained): same files, fewer candidate-row fetches;
     * only the diagnostic k-mer-hit count in the log then counts the compared candidates */
    disco_params prm{min_overlap, 4, DISCO_FLAG_SEEDED_KMER | (getenv("DISCO_EXACT_COUNTERS") ? 0u : DISCO_FLAG_TWO_PASS_VERIFY), max_subs};
    std::unique_ptr<uint16_t[]> edge_subs; /* substitutions per edge (third number of an edge line); stays null with exact overlaps */
    uint64_t n_cont = 0, e_pre = 0, e_out = 0;
    std::vector<disco_contained_row> rows;
    bool rows_grouped = false; /* rows already are in the contained-read files' order (disco_fetch_contained_grouped) */
    std::unique_ptr<disco_edge[]> edges;
    std::unique_ptr<uint16_t[]> edge_file;
    const int n_edge_files = mpi_names ? gpus * std::max(threads - 1, 1) : threads;
    double t_graph = 0, t_h2d = 0;
    t0 = Clock::now();
    auto t1 = Clock::now();
    /* what the writer thread captures by reference comes FIRST: locals die in reverse order of declaration, so the holders below join
     * their threads before any of these goes away on an early return */
    bool contained_early = false, contained_ok = true, edge_text_streamed = false, contained_on_gpu = false;
    std::string contained_err;
    const disco::FileTags ctags_early = mpi_names ? disco::FileTags::mpi_contained(gpus, threads) : disco::FileTags::plain(threads);
    /* (threads declared before anything that may return early: their holders join on the way out) */
    struct ThreadHolder {
        std::thread t;
        ~ThreadHolder()
        {
            if (t.joinable()) t.join();
        }
    } contained_writer_holder, ctx_releaser_holder;
    std::thread &contained_writer = contained_writer_holder.t, &ctx_releaser = ctx_releaser_holder.t;
    auto lap = [&](const char *what) {
        if (verbose) fprintf(stderr, "[disco host] %-28s %.3f s\n", what, secs(t1));
        t1 = Clock::now();
    };
    if (gpus == 1) {
        disco_ctx *ctx = ctx1;
        if (!ctx && disco_create(gpu, &prm, &ctx) < 0) return die(std::string("disco_create: ") + disco_last_error(nullptr));
        if (!ingested) DISCO_CALL(ctx, disco_upload_reads_ragged(ctx, rs.packed, rs.len.data(), rs.size()));
        t_h2d = secs(t0);
        t0 = Clock::now();
        DISCO_CALL(ctx, disco_build_index(ctx));
        DISCO_CALL(ctx, disco_probe(ctx));
        DISCO_CALL(ctx, disco_mark_contained(ctx, &n_cont));
        std::cout << "\n" << (rs.size() - n_cont) << " Non-contained reads. (Keep as is)\n"
                  << n_cont << " contained reads. (Need to change their mate-pair information)" << std::endl;
        /* the contained-read files from the GPU (disco_format_contained: rows grouped, sorted and formatted where the keys are, the lines
         * through the pinned ring into the files) — or, where the rows are wanted on the host (binary side output, no text, DISCO_HOST_TEXT
         * / DISCO_HOST_CONTAINED_TEXT=1), the rows leave now, grouped for their files, while the edges are selected and reduced */
        /* with the binary files written from the device (gpu_binary) the rows are wanted on the host for host-formatted text only, and a
         * --binary-out run keeps the text path of a run without the flag */
        bool gpu_contained = !no_text && (!binary_out || gpu_binary) && !getenv("DISCO_HOST_TEXT") && !getenv("DISCO_HOST_CONTAINED_TEXT");
        const bool rows_wanted = !gpu_contained && !(gpu_binary && no_text);
        if (rows_wanted && n_cont && !getenv("DISCO_HOST_ROW_SORT") && !getenv("DISCO_LATE_ROWS")) (void)disco_start_contained_rows(ctx, 1);
        DISCO_CALL(ctx, disco_build_edges(ctx, &e_pre));
        DISCO_CALL(ctx, disco_transitive_reduce(ctx, &e_out));
        t_graph = secs(t0);
        disco_counters cn;
        DISCO_CALL(ctx, disco_get_counters(ctx, &cn));
        std::cout << "Graph construction complete.\n"
                  << "  overlaps (pre-reduction) : " << e_pre << "\n  edges after reduction    : " << e_out << "\n  k-mer probes             : " << cn.probes
                  << "\n  k-mer hits               : " << cn.kmer_hits << "\n  cap_bind_sites           : " << cn.cap_bind_sites
                  << "\n  asymmetric_pairs         : " << cn.asymmetric_pairs << "\n"
                  << "Function buildOverlapGraph() [GPU] finished in " << t_graph << " Seconds (" << (t_graph > 0 ? e_pre / t_graph : 0)
                  << " overlaps/s); host->device " << t_h2d << " Seconds." << std::endl;
        if (!max_subs && (cn.cap_bind_sites || cn.asymmetric_pairs))
            std::cout << "Note: this input is in the order-dependent regime of the reference (edge cap per k-mer reached or overlaps found from one "
                         "side only); the reference's own result varies with its thread count here."
                      << std::endl;
        t0 = Clock::now();
        t1 = Clock::now();
        if (!join_ingest_fetch()) return die(disco_last_error(ctx));
        lap("wait for lengths + file indices");
        if (gpu_contained) {
            /* right behind the reduction: the ring is free, and nothing of the rows crosses to the host */
            const int ncf = (int)ctags_early.tag.size();
            const bool identity = rs.total_records == rs.size(); /* no record was filtered: file index = read id + 1 */
            std::vector<uint64_t> coff((size_t)ncf + 1, 0);
            const int64_t nb = disco_format_contained(ctx, (uint32_t)ncf, identity ? nullptr : rs.file_index.data(), coff.data());
            if (nb == DISCO_E_NOMEM || nb == DISCO_E_UNSUPPORTED) {
                if (verbose) fprintf(stderr, "[disco host] contained lines by the host writer: %s\n", disco_last_error(ctx));
                gpu_contained = false;
            } else if (nb < 0)
                return die(disco_last_error(ctx));
            else {
                lap("format contained lines on the GPU");
                std::vector<int> fds((size_t)ncf, -1);
                std::string ferr;
                if (!disco::open_contained_files(prefix, ncf, &ctags_early, fds.data(), ferr)) return die(ferr);
                const int wrc = disco_write_contained_text(ctx, fds.data(), (uint32_t)ncf, (uint32_t)threads);
                for (int fd : fds)
                    if (fd >= 0) close(fd);
                if (wrc < 0) return die(disco_last_error(ctx));
                lap("contained lines into the files");
            }
            contained_on_gpu = gpu_contained;
        }
        auto soft = [](int64_t rc) { return rc == DISCO_E_NOMEM || rc == DISCO_E_UNSUPPORTED; };
        const bool identity_ids = rs.total_records == rs.size(); /* no record was filtered: file index = read id + 1 */
        if (gpu_binary) {
            /* <prefix>_contained.bin: the header from here, the records from the device (grouped and sorted there) into the open file */
            const int ncf = (int)ctags_early.tag.size();
            const int64_t nr = disco_prepare_contained_records(ctx, (uint32_t)ncf, identity_ids ? nullptr : rs.file_index.data());
            if (nr < 0 && !soft(nr)) return die(disco_last_error(ctx));
            int wrc = (int)std::min<int64_t>(nr, 0);
            if (nr >= 0) {
                std::string ferr;
                const int fd = disco::open_binary_records(prefix, true, (uint64_t)nr, ncf, ferr);
                if (fd < 0) return die(ferr);
                wrc = disco_write_contained_records(ctx, fd, 32, (uint32_t)threads);
                close(fd);
                if (wrc < 0 && !soft(wrc)) return die(disco_last_error(ctx));
            }
            if (wrc < 0) {
                if (verbose) fprintf(stderr, "[disco host] binary contained records by the host writer: %s\n", disco_last_error(ctx));
            } else {
                bin_contained_on_gpu = true;
                lap("binary contained records on the GPU");
            }
        }
        /* the rows as host records: for host-formatted text and for the host writer of the binary file */
        const bool rows_needed = (!no_text && !gpu_contained) || (binary_out && !bin_contained_on_gpu);
        if (rows_needed) rows.resize(n_cont);
        if (n_cont && rows_needed) { /* in the files' order where the device grouped them during the pass; by id (sorted by the writer) otherwise */
            const int64_t grc = getenv("DISCO_HOST_ROW_SORT") ? (int64_t)DISCO_E_UNSUPPORTED : disco_fetch_contained_grouped(ctx, rows.data(), n_cont);
            rows_grouped = grc >= 0;
            if (grc < 0 && grc != DISCO_E_UNSUPPORTED) return die(disco_last_error(ctx));
            if (!rows_grouped && disco_fetch_contained(ctx, rows.data(), n_cont) < 0) return die(disco_last_error(ctx));
        }
        lap("fetch contained rows");
        /* the contained-read files are written by a thread of their own while the device partitions and formats the edges (their rows
         * have been final since the contained flags were fixed); joined before the checkpoint is written */
        /* (not beside the host writer of the binary file: write_binary_contained sorts the rows in place) */
        if (!no_text && (!binary_out || bin_contained_on_gpu) && !gpu_contained) {
            contained_early = true;
            contained_writer = std::thread([&]() {
                std::string e2;
                contained_ok = disco::write_contained(prefix, (int)ctags_early.tag.size(), rows, rs, e2, &ctags_early, rows_grouped);
                if (!contained_ok) contained_err = e2;
            });
        }
        /* connected components of the reduced graph dealt out to the files: every node has all its edges in one file, which is
         * what lets parsimplify work on the files independently (the reference gets it from its BFS batches) */
        edge_file.reset(new uint16_t[std::max<uint64_t>(e_out, 1)]);
        if (e_out && disco_fetch_edge_files(ctx, (uint32_t)n_edge_files, edge_file.get(), e_out) < 0) return die(disco_last_error(ctx));
        lap("partition edges into files");
        /* the edge lines of the text files formatted where the edges are (2.5 GB of numbers at config 3); DISCO_HOST_TEXT=1: by the host writer */
        if (e_out && !no_text && !max_subs && n_edge_files <= 256 && !getenv("DISCO_HOST_TEXT")) {
            const bool identity = rs.total_records == rs.size(); /* no record was filtered: file index = read id + 1 */
            edge_text_off.assign((size_t)n_edge_files + 1, 0);
            const int64_t nb = disco_format_edges(ctx, (uint32_t)n_edge_files, edge_file.get(), identity ? nullptr : rs.file_index.data(), edge_text_off.data());
            if (nb < 0) return die(disco_last_error(ctx));
            lap("format edge lines on the GPU");
            if ((!binary_out || gpu_binary) && (par_simple.empty() || par_simple_on_gpu) && !getenv("DISCO_TEXT_VIA_HOST")) {
                /* straight from the device into the edge files (pieces through a pinned ring, host threads pwrite behind the copies) */
                const disco::FileTags et = mpi_names ? disco::FileTags::mpi_edges(gpus, threads) : disco::FileTags::plain(threads);
                std::vector<int> fds((size_t)n_edge_files, -1);
                std::string ferr;
                if (!disco::open_edge_files(prefix, (int)n_edge_files, &et, rs.size(), fds.data(), ferr)) return die(ferr);
                const int wrc = disco_write_edge_text(ctx, fds.data(), (uint32_t)n_edge_files, (uint32_t)threads);
                for (int fd : fds)
                    if (fd >= 0) close(fd);
                if (wrc < 0) return die(disco_last_error(ctx));
                edge_text_streamed = true;
                lap("edge lines into the files");
            } else {
                edge_text.reset(new char[std::max<int64_t>(nb, 1)]);
                DISCO_CALL(ctx, disco_fetch_edge_text(ctx, edge_text.get(), (uint64_t)nb));
                lap("fetch edge lines");
            }
        }
        /* the edges as host records: only for what still works on them there (binary side output, partial simplification, host-formatted text) */
        auto fetch_edges = [&]() -> bool {
            edges.reset(new disco_edge[std::max<uint64_t>(e_out, 1)]); /* 1.8 GB at 45 M edges: not zero-filled first */
            if (e_out && disco_fetch_edges(ctx, edges.get(), e_out) < 0) return false;
            if (max_subs) {
                edge_subs.reset(new uint16_t[std::max<uint64_t>(e_out, 1)]);
                if (e_out && disco_fetch_edge_substitutions(ctx, edge_subs.get(), e_out) < 0) return false;
            }
            lap("fetch edges");
            return true;
        };
        if (gpu_binary) {
            /* <prefix>_edges.bin the same way: any number of files, substitutions included (the edge TEXT of such runs stays with the host writer) */
            const int64_t nr = disco_prepare_edge_records(ctx, (uint32_t)n_edge_files, edge_file.get(), identity_ids ? nullptr : rs.file_index.data());
            if (nr < 0 && !soft(nr)) return die(disco_last_error(ctx));
            int wrc = (int)std::min<int64_t>(nr, 0);
            if (nr >= 0) {
                std::string ferr;
                const int fd = disco::open_binary_records(prefix, false, (uint64_t)nr, n_edge_files, ferr);
                if (fd < 0) return die(ferr);
                wrc = disco_write_edge_records(ctx, fd, 32, (uint32_t)threads);
                close(fd);
                if (wrc < 0 && !soft(wrc)) return die(disco_last_error(ctx));
            }
            if (wrc < 0) {
                if (verbose) fprintf(stderr, "[disco host] binary edge records by the host writer: %s\n", disco_last_error(ctx));
            } else {
                bin_edges_on_gpu = true;
                lap("binary edge records on the GPU");
            }
        }
        if ((binary_out && !bin_edges_on_gpu) || (!par_simple.empty() && !par_simple_on_gpu) || (!edge_text && !edge_text_streamed && !no_text))
            if (!fetch_edges()) return die(disco_last_error(ctx));
        if (par_simple_on_gpu && e_out) {
            /* contract -> residue, headers, first edges -> the host rounds on that small graph -> the lines from the device into the files.
             * A call that has no memory or does not support the case hands the run back to the flow through the host, below */
            uint64_t nc = 0, nl = 0;
            DISCO_CALL(ctx, disco_contract_chains(ctx, min_overlap_simplify, &nc, &nl));
            const int n_ps_files = threads;
            auto give_up = [&](const char *what) {
                if (verbose) fprintf(stderr, "[disco host] partial simplification through the host: %s: %s\n", what, disco_last_error(ctx));
                par_simple_on_gpu = false;
            };
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
            if (soft(rc)) give_up("fetching the residue");
            else if (rc < 0) return die(disco_last_error(ctx));
            lap("contract chains on the GPU");
            if (par_simple_on_gpu) {
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
                if (!disco::write_par_simple_residue(par_simple, n_ps_files, res, rs, err, &ps, nullptr, nullptr, &desc)) return die(err);
                lap("partial simplification: host rounds");
                const bool identity = rs.total_records == rs.size();
                std::vector<uint64_t> poff((size_t)n_ps_files + 1, 0);
                const int64_t nb = disco_format_par_simple(ctx, (uint32_t)n_ps_files, identity ? nullptr : rs.file_index.data(), desc.edges.data(), desc.edges.size(),
                                                           desc.pieces.data(), desc.pieces.size(), poff.data());
                if (soft(nb)) give_up("formatting the lines");
                else if (nb < 0) return die(disco_last_error(ctx));
                else {
                    if (verbose)
                        fprintf(stderr, "[disco host] partial simplification on the GPU: residue %lld edges + %llu composite edges -> %zu final edges in %zu pieces (%llu reversed, at most %u in one edge), %lld bytes of text\n",
                                (long long)nres, (unsigned long long)nc, desc.edges.size(), desc.pieces.size(), (unsigned long long)desc.reversed_pieces, desc.max_pieces, (long long)nb);
                    const disco::FileTags pt = disco::FileTags::plain(threads);
                    std::vector<int> fds((size_t)n_ps_files, -1);
                    bool opened = true;
                    for (int t = 0; t < n_ps_files && opened; t++) {
                        const std::string path = par_simple + "_" + pt.tag[(size_t)t] + "_ParSimpleEdges.txt";
                        fds[(size_t)t] = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
                        if (fds[(size_t)t] < 0) {
                            opened = false;
                            err = "Unable to write file: " + path;
                        }
                    }
                    const int wrc = opened ? disco_write_par_simple_text(ctx, fds.data(), (uint32_t)n_ps_files, (uint32_t)threads) : 0;
                    for (int fd : fds)
                        if (fd >= 0) close(fd);
                    if (!opened) return die(err);
                    if (wrc < 0) return die(disco_last_error(ctx));
                    std::cout << "Partial simplification (the reference's parsimplify step) on the resident graph: " << ps.edges_in << " edges -> " << ps.edges_out << " ("
                              << ps.nodes_absorbed << " nodes absorbed into composite edges, " << ps.dead_end_nodes << " dead-end nodes, " << ps.rounds << " rounds); files "
                              << par_simple << "_<i>_ParSimpleEdges.txt" << std::endl;
                    lap("partial simplification");
                    par_simple_done = true;
                }
            }
            if (!par_simple_on_gpu) { /* handed back: what the flow through the host works on */
                if (!edges && !fetch_edges()) return die(disco_last_error(ctx));
                ch_links.reset(new disco_chain_link[std::max<uint64_t>(nl, 1)]);
                ch_absorbed.reset(new uint8_t[e_out]);
                DISCO_CALL(ctx, disco_fetch_chains(ctx, ch_comp.data(), ch_links.get(), ch_absorbed.get()));
            }
        } else if (gpu_chains && e_out) {
            uint64_t nc = 0, nl = 0;
            DISCO_CALL(ctx, disco_contract_chains(ctx, min_overlap_simplify, &nc, &nl));
            ch_comp.resize(nc);
            ch_links.reset(new disco_chain_link[std::max<uint64_t>(nl, 1)]);
            ch_absorbed.reset(new uint8_t[e_out]);
            DISCO_CALL(ctx, disco_fetch_chains(ctx, ch_comp.data(), ch_links.get(), ch_absorbed.get()));
            lap("contract chains on the GPU");
        }
        /* the context is released by a thread of its own while the files are written (0.07 s of hipFree at config 3) */
        ctx_releaser = std::thread([ctx]() { disco_destroy(ctx); });
        lap("release GPU context (in the background)");
    } else {
        /* one rank per GPU, one host thread per rank (replaces mpirun -np N of runDisco-MPI.sh:214-258): rank r holds the reads
         * [r*per, (r+1)*per), every exchange is an RCCL collective inside libdisco_hip.so */
        std::vector<RankResult> res((size_t)gpus);
        std::vector<std::thread> th;
        /* every rank writes its share of the text files from its GPU — under the conditions of the single-GPU device path: text is wanted and
         * nothing else needs the records on the host (no binary side output, no partial simplification), exact overlaps, at most 256 edge
         * files, no DISCO_HOST_TEXT (DISCO_HOST_CONTAINED_TEXT: the contained files alone stay with the host writer).
         * Opt-in: DISCO_DIST_GPU_TEXT=1 (DIST_GPU_TEXT_DEFAULT above says why); unset or 0: the host writer for both kinds */
        const char *dgt = getenv("DISCO_DIST_GPU_TEXT");
        const bool dev_text_wanted = (dgt ? strcmp(dgt, "0") != 0 : DIST_GPU_TEXT_DEFAULT) && !no_text && !binary_out && par_simple.empty() && !max_subs && !getenv("DISCO_HOST_TEXT") &&
                                     !getenv("DISCO_TEXT_VIA_HOST");
        const bool dev_contained_wanted = dev_text_wanted && !getenv("DISCO_HOST_CONTAINED_TEXT");
        const bool dev_edges_wanted = dev_text_wanted && n_edge_files <= 256;
        const std::vector<uint64_t> woff = ingested ? std::vector<uint64_t>() : rs.word_offsets();
        if (ctx.empty())
            if (const std::string e = make_ranks(); !e.empty()) return die(e);
        wd_paused.store(false);
        for (int r = 0; r < gpus; r++)
            th.emplace_back([&, r]() {
                RankResult &R = res[(size_t)r];
                disco_ctx *c = ctx[(size_t)r];
                auto at = [&](int x) { stage[(size_t)r].store(x); };
                auto bail = [&](const char *what) {
                    R.err = std::string(what) + ": " + disco_last_error(c);
                    /* the other ranks wait for this one inside a collective: there is nothing to unwind to */
                    std::cout << "\nError (rank " << r << "): " << R.err << std::endl;
                    _exit(2);
                };
                if (!comm_joined) {
                    at(ST_COMM_INIT);
                    if (!same_device && disco_comm_init(c, uid, gpus, r) < 0) bail("disco_comm_init");
                }
                if (!ingested) { /* (the device input stage left the rank's home range in place, as the upload does) */
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
                if (disco_dist_run_graph(c, DISCO_DIST_GATHER_READS | (partitioned_index ? DISCO_DIST_KEEP_INDEX_PARTITIONED : 0)) < 0) bail("disco_dist_run_graph");
                if (disco_dist_get_info(c, &R.info) < 0) bail("disco_dist_get_info");
                if (verbose && r == 0) fprintf(stderr, "[disco host] transport %s, %d ranks\n", disco_comm_kind(c), gpus);
                R.pass_end = Clock::now();
                /* The rank's share of the files from its GPU: the files f of a kind with floor(f gpus / files) == r. Both calls are collective
                 * and end alike on every rank, so the ranks take the same way without asking each other: all of them write their files, or —
                 * DISCO_E_UNSUPPORTED / DISCO_E_NOMEM — all of them hand their rows / edges to the host writer below, in the same run */
                auto t_lap = Clock::now();
                auto rank_lap = [&](const char *what) {
                    if (verbose) fprintf(stderr, "[disco host] rank %d: %-36s %.3f s\n", r, what, secs(t_lap));
                    t_lap = Clock::now();
                };
                const bool identity = rs.total_records == rs.size(); /* no record was filtered: file index = read id + 1 */
                auto own_files = [&](int n_files, int *lo, int *hi) {
                    *lo = (int)(((int64_t)r * n_files + gpus - 1) / gpus);
                    *hi = (int)(((int64_t)(r + 1) * n_files + gpus - 1) / gpus);
                };
                auto close_all = [](std::vector<int> &fds) {
                    for (int fd : fds)
                        if (fd >= 0) close(fd);
                };
                R.dev_contained = dev_contained_wanted;
                if (R.dev_contained) {
                    at(ST_FORMAT_CONTAINED);
                    const int ncf = (int)ctags_early.tag.size();
                    std::vector<uint64_t> coff((size_t)ncf + 1, 0);
                    const int64_t nb = disco_dist_format_contained(c, (uint32_t)ncf, identity ? nullptr : rs.file_index.data(), coff.data());
                    if (nb == DISCO_E_NOMEM || nb == DISCO_E_UNSUPPORTED) {
                        if (verbose) fprintf(stderr, "[disco host] rank %d: contained lines by the host writer: %s\n", r, disco_last_error(c));
                        R.dev_contained = false;
                    } else if (nb < 0)
                        bail("disco_dist_format_contained");
                    else {
                        rank_lap("format contained lines on the GPU");
                        at(ST_WRITE_CONTAINED);
                        int lo, hi;
                        own_files(ncf, &lo, &hi);
                        std::vector<int> fds((size_t)ncf, -1);
                        std::string ferr;
                        if (!disco::open_contained_files(prefix, ncf, &ctags_early, fds.data(), ferr, lo, hi)) {
                            std::cout << "\nError (rank " << r << "): " << ferr << std::endl;
                            _exit(2);
                        }
                        const int wrc = disco_write_contained_text(c, fds.data(), (uint32_t)ncf, (uint32_t)threads);
                        close_all(fds);
                        if (wrc < 0) bail("disco_write_contained_text");
                        rank_lap("contained lines into the files");
                    }
                }
                if (!R.dev_contained) {
                    at(ST_FETCH_CONTAINED);
                    R.rows.resize(R.info.n_contained_local);
                    if (R.info.n_contained_local && disco_fetch_contained(c, R.rows.data(), R.info.n_contained_local) < 0) bail("disco_fetch_contained");
                }
                R.dev_edges = dev_edges_wanted;
                if (R.dev_edges) {
                    at(ST_FORMAT_EDGES);
                    std::vector<uint64_t> eoff((size_t)n_edge_files + 1, 0);
                    const int64_t nb = disco_dist_format_edges(c, (uint32_t)n_edge_files, identity ? nullptr : rs.file_index.data(), eoff.data());
                    if (nb == DISCO_E_NOMEM || nb == DISCO_E_UNSUPPORTED) {
                        if (verbose) fprintf(stderr, "[disco host] rank %d: edge lines by the host writer: %s\n", r, disco_last_error(c));
                        R.dev_edges = false;
                    } else if (nb < 0)
                        bail("disco_dist_format_edges");
                    else {
                        rank_lap("partition + format edge lines on the GPU");
                        at(ST_WRITE_EDGES);
                        int lo, hi;
                        own_files(n_edge_files, &lo, &hi);
                        const disco::FileTags et = mpi_names ? disco::FileTags::mpi_edges(gpus, threads) : disco::FileTags::plain(threads);
                        std::vector<int> fds((size_t)n_edge_files, -1);
                        std::string ferr;
                        if (!disco::open_edge_files(prefix, n_edge_files, &et, rs.size(), fds.data(), ferr, lo, hi)) {
                            std::cout << "\nError (rank " << r << "): " << ferr << std::endl;
                            _exit(2);
                        }
                        const int wrc = disco_write_edge_text(c, fds.data(), (uint32_t)n_edge_files, (uint32_t)threads);
                        close_all(fds);
                        if (wrc < 0) bail("disco_write_edge_text");
                        rank_lap("edge lines into the files");
                    }
                }
                if (!R.dev_edges) {
                    at(ST_FETCH_EDGES);
                    R.n_edges = R.info.e_out_local;
                    R.edges.reset(new disco_edge[std::max<uint64_t>(R.n_edges, 1)]);
                    if (R.n_edges && disco_fetch_edges(c, R.edges.get(), R.n_edges) < 0) bail("disco_fetch_edges");
                    if (max_subs) {
                        R.subs.reset(new uint16_t[std::max<uint64_t>(R.n_edges, 1)]);
                        if (R.n_edges && disco_fetch_edge_substitutions(c, R.subs.get(), R.n_edges) < 0) bail("disco_fetch_edge_substitutions");
                    }
                }
                at(ST_DONE);
            });
        for (auto &t : th) t.join();
        ranks_done.store(true);
        const bool dev_contained = res[0].dev_contained, dev_edges = res[0].dev_edges;
        for (auto &R : res)
            if (R.dev_contained != dev_contained || R.dev_edges != dev_edges) return die("the ranks disagree about who writes the text files");
        /* (where the ranks wrote files, the graph was complete when the last rank left the pass: what they did behind it is output stage) */
        auto t_pass_end = Clock::now();
        if (dev_contained || dev_edges) {
            t_pass_end = res[0].pass_end;
            for (auto &R : res) t_pass_end = std::max(t_pass_end, R.pass_end);
        }
        t_graph = std::chrono::duration<double>(t_pass_end - t0).count();
        const disco_dist_info &di = res[0].info;
        n_cont = di.n_contained;
        e_pre = di.e_pre;
        e_out = di.e_out;
        std::cout << "\n" << (rs.size() - n_cont) << " Non-contained reads. (Keep as is)\n"
                  << n_cont << " contained reads. (Need to change their mate-pair information)" << std::endl;
        std::cout << "Graph construction complete on " << gpus << " ranks" << (same_device ? " (one device, in-process exchanges)" : " (RCCL)") << ".\n"
                  << "  overlaps (pre-reduction) : " << e_pre << "\n  edges after reduction    : " << e_out << "\n  k-mer probes             : " << di.probes
                  << "\n  k-mer hits               : " << di.kmer_hits << "\n  cap_bind_sites           : " << di.cap_bind_sites
                  << "\n  asymmetric_pairs         : " << di.asymmetric_pairs << "\n  regime                   : "
                  << (di.regime == 0   ? "regular (neighbour rows on request)"
                      : di.regime == 2 ? "regular after completing the lists of the reads that dropped a hit across ranks"
                                       : "order-dependent (adjacency gathered)")
                  << "\n"
                  << "Function buildOverlapGraph() [" << gpus << " GPU ranks] finished in " << t_graph << " Seconds incl. upload (" << (t_graph > 0 ? e_pre / t_graph : 0)
                  << " overlaps/s); last pass " << di.ms_total * 1e-3 << " Seconds on rank 0." << std::endl;
        if (!max_subs && (di.cap_bind_sites || di.asymmetric_pairs))
            std::cout << "Note: this input is in the order-dependent regime of the reference (edge cap per k-mer reached or overlaps found from one "
                         "side only); the reference's own result varies with its thread count here."
                      << std::endl;
        t0 = dev_contained || dev_edges ? t_pass_end : Clock::now();
        t1 = Clock::now();
        if (verbose && (dev_contained || dev_edges)) fprintf(stderr, "[disco host] %-28s %.3f s\n", "text files by the ranks", secs(t_pass_end));
        contained_on_gpu = dev_contained;
        edge_text_streamed = dev_edges;
        /* the ranks' shares side by side: contained rows of rank r's reads, edges whose smaller endpoint rank r owns */
        uint64_t nr = 0, ne = 0;
        for (auto &R : res) {
            nr += R.rows.size();
            ne += R.n_edges;
        }
        if ((!dev_contained && nr != n_cont) || (!dev_edges && ne != e_out)) return die("the ranks' shares do not add up to the job's totals");
        rows.reserve(nr);
        for (auto &R : res) {
            rows.insert(rows.end(), R.rows.begin(), R.rows.end());
            std::vector<disco_contained_row>().swap(R.rows);
        }
        edges.reset(new disco_edge[std::max<uint64_t>(ne, 1)]);
        if (max_subs) edge_subs.reset(new uint16_t[std::max<uint64_t>(ne, 1)]);
        uint64_t at = 0;
        for (auto &R : res) {
            if (R.n_edges) memcpy(edges.get() + at, R.edges.get(), R.n_edges * sizeof(disco_edge));
            if (R.n_edges && max_subs) memcpy(edge_subs.get() + at, R.subs.get(), R.n_edges * sizeof(uint16_t));
            at += R.n_edges;
            R.edges.reset();
            R.subs.reset();
        }
        lap("gather the ranks' shares");
        if (!dev_edges) {
            edge_file.reset(new uint16_t[std::max<uint64_t>(e_out, 1)]);
            if (e_out && disco_partition_edges(ctx[0], edges.get(), e_out, rs.size(), (uint32_t)n_edge_files, edge_file.get()) < 0) return die(disco_last_error(ctx[0]));
            lap("partition edges into files");
        }
        if (gpu_chains && e_out) { /* the ranks' edges lie on the host: rank 0's context, which holds every read's length, contracts them */
            uint64_t nc = 0, nl = 0;
            DISCO_CALL(ctx[0], disco_contract_chains_of(ctx[0], edges.get(), e_out, min_overlap_simplify, &nc, &nl));
            ch_comp.resize(nc);
            ch_links.reset(new disco_chain_link[std::max<uint64_t>(nl, 1)]);
            ch_absorbed.reset(new uint8_t[e_out]);
            DISCO_CALL(ctx[0], disco_fetch_chains(ctx[0], ch_comp.data(), ch_links.get(), ch_absorbed.get()));
            lap("contract chains on the GPU");
        }
        for (auto c : ctx) disco_destroy(c);
        lap("release GPU contexts");
    }

    /* ---- outputs -------------------------------------------------------------------------------------------------- */
    disco::FileTags etags = mpi_names ? disco::FileTags::mpi_edges(gpus, threads) : disco::FileTags::plain(threads);
    disco::FileTags ctags = mpi_names ? disco::FileTags::mpi_contained(gpus, threads) : disco::FileTags::plain(threads);
    if (binary_out && !(bin_edges_on_gpu && bin_contained_on_gpu)) { /* (a file the device has written is left alone) */
        if (!bin_edges_on_gpu && !disco::write_binary_edges(prefix, (int)etags.tag.size(), edges.get(), e_out, e_out ? edge_file.get() : nullptr, rs, err, edge_subs.get()))
            return die(err);
        if (!bin_contained_on_gpu && !disco::write_binary_contained(prefix, (int)ctags.tag.size(), rows, rs, err)) return die(err);
        lap("write binary side output");
    }
    if (!par_simple.empty() && !mpi_names && !par_simple_done) {
        disco::ParSimpleStats ps;
        disco::ChainSeed seed;
        if (ch_absorbed) {
            seed.comp = ch_comp.data();
            seed.n_comp = ch_comp.size();
            seed.links = ch_links.get();
            seed.absorbed = ch_absorbed.get();
        }
        if (!disco::write_par_simple(par_simple, (int)etags.tag.size(), edges.get(), e_out, e_out ? edge_file.get() : nullptr, rs, min_overlap_simplify, threads, err, &ps,
                                     nullptr, nullptr, nullptr, ch_absorbed ? &seed : nullptr))
            return die(err);
        std::cout << "Partial simplification (the reference's parsimplify step) on the resident graph: " << ps.edges_in << " edges -> " << ps.edges_out << " ("
                  << ps.nodes_absorbed << " nodes absorbed into composite edges, " << ps.dead_end_nodes << " dead-end nodes, " << ps.rounds << " rounds); files "
                  << par_simple << "_<i>_ParSimpleEdges.txt" << std::endl;
        lap("partial simplification");
    }
    if (no_text) { /* the file lists of the scripts still exist (the consumer aborts on a missing file), empty */
        rows.clear();
        e_out = 0;
    }
    if (contained_on_gpu) { /* written while the text left the device */
    } else if (contained_early) {
        contained_writer.join();
        if (!contained_ok) return die(contained_err);
    } else if (!disco::write_contained(prefix, (int)ctags.tag.size(), rows, rs, err, &ctags, rows_grouped))
        return die(err);
    lap("write contained rows");
    if (!disco::write_checkpoint(prefix, true, false, false, err)) return die(err);
    if (edge_text_streamed && !no_text) { /* written while the text left the device */
    } else if (edge_text && !no_text) {
        if (!disco::write_edge_text(prefix, (int)etags.tag.size(), edge_text.get(), edge_text_off.data(), rs.size(), err, &etags)) return die(err);
    } else if (!disco::write_edges(prefix, (int)etags.tag.size(), edges.get(), e_out, rs, threads, err, e_out ? edge_file.get() : nullptr, &etags, edge_subs.get()))
        return die(err);
    lap("write edges");
    if (!disco::write_checkpoint(prefix, false, true, true, err)) return die(err);
    /* every file is written and closed, the checkpoint says so: the stage is over. What is left is tearing down the GPU runtime — tens of
     * GB of device memory, its streams and events, the libraries' static state: 0.15-0.2 s at config 3 that produce nothing (the
     * driver takes everything back when the process ends, whichever way it ends). DISCO_ORDERLY_EXIT=1 keeps the long way (leak
     * checkers, tests that want the destructors to run). */
    /* round 6: the orderly way is the DEFAULT whenever somebody may be listening at exit — a profiler or tracer preloaded into the
     * process (rocprofv3 / roctx write their output from atexit handlers and tool finalizers: `rocprofv3 --marker-trace -- buildG ...` of
     * DESIGN.md section 1 lost its trace to the quick exit), LD_PRELOAD in general, coverage and sanitizer runtimes, DISCO_TRACE — and the
     * releaser thread is JOINED before either exit: leaving through _exit while it sits inside disco_destroy / hipFree raced the runtime's
     * own teardown. DISCO_QUICK_EXIT=1 forces the short way, DISCO_ORDERLY_EXIT=1 the long one. */
    const bool tool_attached = getenv("ROCP_TOOL_LIBRARIES") || getenv("ROCPROFILER_REGISTER_FORCE_LOAD") || getenv("HSA_TOOLS_LIB") || getenv("LD_PRELOAD") ||
                               getenv("DISCO_TRACE") || getenv("GCOV_PREFIX") || getenv("ASAN_OPTIONS") || getenv("TSAN_OPTIONS") || getenv("UBSAN_OPTIONS");
    const bool orderly = getenv("DISCO_ORDERLY_EXIT") != nullptr || (tool_attached && !getenv("DISCO_QUICK_EXIT"));
    std::cout << "Function saveParGraphToFile() finished in " << secs(t0) << " Seconds." << std::endl;
    std::cout << "Function main() finished in " << secs(t_main) << " Seconds." << std::endl;
    if (ctx_releaser.joinable()) ctx_releaser.join(); /* (0.07 s of hipFree at config 3, nearly all of it behind the writers by now) */
    if (!orderly) {
        std::cout.flush();
        std::cerr.flush();
        fflush(nullptr);
        _exit(0);
    }
    return 0;
}
