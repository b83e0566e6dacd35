/*
 * plan_check — buildG's output plan (output_plan.h) walked exhaustively on the host, for tests/test_output_plan_host.py.
 *   plan_check knobs : "<variable> <unset> <"0"> <"1">" per routing variable: what read_knobs() makes of the three settings
 *   plan_check       : one line "<fields>" per combination, in the order of the loops below (the last loop runs fastest):
 *                        gpus {1,2} x output {text, --binary-out, --no-text} x par_simple x mpi_names x max_subs x n_edge_files {256,257}
 *                        x the seven flags {off,on} x the three tri-states {unset,"0","1"}
 *                      then one line "<options> <fields> <demoted> <fields after>" for every plan that occurs under those options and every
 *                      set of its Device products demoted (plan() sees the knobs' values only and demote() the plan only, so the strings of
 *                      the first mode and the plans of this one cover the product of both)
 * <fields>, in hex: 2 bits per product (contained text, edge text, _contained.bin, _edges.bin, ParSimpleEdges; 0 none, 1 device, 2 host), then
 * one bit each: chains on device, rows early, rows grouped, edge text streamed, rows on host, contained text by the writer thread, edges on host.
 */
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <utility>

#include "output_plan.h"

using namespace disco;

static unsigned fields(const OutputPlan &p)
{
    unsigned m = 0;
    for (int i = 0; i < N_PRODUCTS; i++) m |= (unsigned)p.maker[i] << (2 * i);
    const bool bits[] = {p.chains_on_device, p.rows_early, p.rows_grouped, p.edge_text_streamed(), p.rows_on_host(), p.contained_by_writer_thread(), p.edges_on_host()};
    for (int i = 0; i < 7; i++) m |= (unsigned)bits[i] << (10 + i);
    return m;
}

static const char *g_name = nullptr, *g_value = nullptr; /* the one variable plan_check's environment holds */
static char *fake_env(const char *name) { return g_name && g_value && !strcmp(name, g_name) ? const_cast<char *>(g_value) : nullptr; }

static int knobs_mode()
{
    struct {
        const char *name;
        int (*get)(const Knobs &);
    } const all[] = {
        {"DISCO_HOST_TEXT", [](const Knobs &k) -> int { return k.host_text; }},
        {"DISCO_HOST_CONTAINED_TEXT", [](const Knobs &k) -> int { return k.host_contained_text; }},
        {"DISCO_TEXT_VIA_HOST", [](const Knobs &k) -> int { return k.text_via_host; }},
        {"DISCO_LATE_ROWS", [](const Knobs &k) -> int { return k.late_rows; }},
        {"DISCO_HOST_ROW_SORT", [](const Knobs &k) -> int { return k.host_row_sort; }},
        {"DISCO_PAR_SIMPLE_HOST", [](const Knobs &k) -> int { return k.par_simple_host; }},
        {"DISCO_PAR_SIMPLE_HOST_TEXT", [](const Knobs &k) -> int { return k.par_simple_host_text; }},
        {"DISCO_HOST_INPUT", [](const Knobs &k) -> int { return k.host_input; }},
        {"DISCO_PAR_SIMPLE", [](const Knobs &k) -> int { return k.par_simple_env; }},
        {"DISCO_GPU_BINARY", [](const Knobs &k) -> int { return k.gpu_binary; }},
        {"DISCO_PAR_SIMPLE_GPU_TEXT", [](const Knobs &k) -> int { return k.par_simple_gpu_text; }},
        {"DISCO_DIST_GPU_TEXT", [](const Knobs &k) -> int { return k.dist_gpu_text; }},
        {"DISCO_DIST_DEVICE_INPUT", [](const Knobs &k) -> int { return k.dist_device_input; }},
    };
    static const char *const setting[] = {nullptr, "0", "1"};
    for (const auto &v : all) {
        printf("%s", v.name);
        g_name = v.name;
        for (const char *s : setting) {
            g_value = s;
            printf(" %d", v.get(read_knobs(fake_env)));
        }
        printf("\n");
        for (const auto &other : all) { /* ... and no other variable moves it */
            g_name = other.name;
            g_value = "1";
            if (other.name != v.name && v.get(read_knobs(fake_env)) != v.get(Knobs())) return 1;
        }
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "knobs")) return knobs_mode();
    std::string out;
    std::set<std::pair<int, unsigned>> seen; /* (options, plan) */
    std::string demotions;
    char buf[64];
    int oi = 0;
    for (int gpus = 1; gpus <= 2; gpus++)
        for (int output = 0; output < 3; output++)
            for (int ob = 0; ob < 16; ob++, oi++) {
                Options o;
                o.gpus = gpus;
                o.threads = 3;
                o.binary_out = output >= 1;
                o.no_text = output == 2;
                o.par_simple = ob & 8;
                o.mpi_names = ob & 4;
                o.max_subs = ob & 2;
                o.count_files();
                o.n_edge_files = 256 + (ob & 1);
                for (int f = 0; f < 128; f++)
                    for (int t = 0; t < 27; t++) {
                        Knobs k;
                        k.host_text = f & 64;
                        k.host_contained_text = f & 32;
                        k.text_via_host = f & 16;
                        k.late_rows = f & 8;
                        k.host_row_sort = f & 4;
                        k.par_simple_host = f & 2;
                        k.par_simple_host_text = f & 1;
                        k.gpu_binary = (Tri)(t / 9 - 1);
                        k.par_simple_gpu_text = (Tri)(t / 3 % 3 - 1);
                        k.dist_gpu_text = (Tri)(t % 3 - 1);
                        const OutputPlan p = plan(o, k);
                        const unsigned m = fields(p);
                        snprintf(buf, sizeof buf, "%05x\n", m);
                        out += buf;
                        if (!seen.insert({oi, m}).second) continue;
                        for (unsigned d = 0; d < (1u << N_PRODUCTS); d++) { /* every set of its Device products */
                            OutputPlan q = p;
                            bool reachable = true;
                            for (int i = 0; i < N_PRODUCTS; i++)
                                if (d >> i & 1) {
                                    reachable = reachable && q.device((Product)i);
                                    q.demote((Product)i);
                                }
                            if (!reachable) continue;
                            snprintf(buf, sizeof buf, "%02x %05x %02x %05x\n", oi, m, d, fields(q));
                            demotions += buf;
                        }
                    }
            }
    fwrite(out.data(), 1, out.size(), stdout);
    fwrite(demotions.data(), 1, demotions.size(), stdout);
    return 0;
}
