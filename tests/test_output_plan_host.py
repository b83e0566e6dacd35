"""CPU: buildG's output plan (disco_amd/host/output_plan.h) behind disco_amd/bin/plan_check, held to the route table of INTEGRATION.md ("Who
writes which file"), restated here from the table with one array axis per option and knob. plan() sees the knobs' values only and demote()
the plan only, so the check has three parts that together cover the product of options, knob settings and demotions: what read_knobs() makes
of every variable unset / "0" / "1"; the plan of every combination of options and knob values; and every set of demotions of every plan that
occurs under each combination of options."""
import os
import subprocess

import numpy as np

from disco_amd import build

BIN = os.path.join(os.path.dirname(build.HERE), "disco_amd", "bin")
FLAGS = ("HOST_TEXT", "HOST_CONTAINED_TEXT", "TEXT_VIA_HOST", "LATE_ROWS", "HOST_ROW_SORT", "PAR_SIMPLE_HOST", "PAR_SIMPLE_HOST_TEXT")
TRIS = ("GPU_BINARY", "PAR_SIMPLE_GPU_TEXT", "DIST_GPU_TEXT")
AXES = ("gpus", "output", "par_simple", "mpi_names", "max_subs", "n_edge_files") + FLAGS + TRIS   # plan_check's loops, the last one fastest
SHAPE = (2, 3, 2, 2, 2, 2) + (2,) * len(FLAGS) + (3,) * len(TRIS)
NONE, DEVICE, HOST = 0, 1, 2
PRODUCTS = ("contained_text", "edge_text", "contained_bin", "edges_bin", "par_simple_edges")
BITS = ("chains", "rows_early", "rows_grouped", "streamed", "rows_on_host", "writer_thread", "edges_on_host")


def _axis(name):
    """the values along one axis, shaped to broadcast against the others"""
    i = AXES.index(name)
    return np.arange(SHAPE[i]).reshape([-1 if j == i else 1 for j in range(len(SHAPE))])


def _tri(name, default):
    v = _axis(name)   # 0 unset, 1 "0", 2 anything else
    return np.where(v == 0, default, v == 2)


def _by(wanted, on_device):
    return np.where(wanted, np.where(on_device, DEVICE, HOST), NONE)


def _derived(o, maker, streamed_as_planned):
    """what follows from the current routes"""
    dev = {p: maker[p] == DEVICE for p in PRODUCTS}
    return {"streamed": dev["edge_text"] & streamed_as_planned,
            "rows_on_host": (~o["no_text"] & ~dev["contained_text"]) | (o["binary_out"] & ~dev["contained_bin"]),
            "writer_thread": o["single"] & ~o["no_text"] & (~o["binary_out"] | dev["contained_bin"]) & ~dev["contained_text"],
            "edges_on_host": (o["binary_out"] & ~dev["edges_bin"]) | (o["par_simple"] & ~dev["par_simple_edges"]) | (~o["no_text"] & ~dev["edge_text"])}


def _pack(maker, bits):
    m = sum(np.asarray(maker[p], dtype=np.int64) << (2 * i) for i, p in enumerate(PRODUCTS))
    return m + sum(np.asarray(bits[b], dtype=np.int64) << (10 + i) for i, b in enumerate(BITS))


def _options(gpus, output, par_simple, mpi_names):
    return {"single": gpus == 0, "binary_out": output >= 1, "no_text": output == 2, "par_simple": par_simple == 1, "mpi_names": mpi_names == 1}


def _table():
    """the route table, every combination at once"""
    o = _options(*(_axis(a) for a in AXES[:4]))
    max_subs, few_files = _axis("max_subs") == 1, _axis("n_edge_files") == 0   # 256 / 257 edge files
    flag = {f: _axis(f) == 1 for f in FLAGS}
    single, no_text, binary_out, par_simple = o["single"], o["no_text"], o["binary_out"], o["par_simple"]
    ps_files = par_simple & ~o["mpi_names"]
    chains = ps_files & ~flag["PAR_SIMPLE_HOST"]
    # one GPU
    ps_dev = chains & ~max_subs & ~flag["PAR_SIMPLE_HOST_TEXT"] & _tri("PAR_SIMPLE_GPU_TEXT", True)
    bin_dev = binary_out & _tri("GPU_BINARY", no_text)
    c_dev = ~no_text & (~binary_out | bin_dev) & ~flag["HOST_TEXT"] & ~flag["HOST_CONTAINED_TEXT"]
    e_dev = ~no_text & ~max_subs & few_files & ~flag["HOST_TEXT"]
    rows_early = ~c_dev & ~(bin_dev & no_text) & ~flag["HOST_ROW_SORT"] & ~flag["LATE_ROWS"]
    stream = (~binary_out | bin_dev) & (~par_simple | ps_dev) & ~flag["TEXT_VIA_HOST"]
    # ranks
    r_text = _tri("DIST_GPU_TEXT", False) & ~no_text & ~binary_out & ~par_simple & ~max_subs & ~flag["HOST_TEXT"] & ~flag["TEXT_VIA_HOST"]
    maker = {"contained_text": _by(~no_text, np.where(single, c_dev, r_text & ~flag["HOST_CONTAINED_TEXT"])),
             "edge_text": _by(~no_text, np.where(single, e_dev, r_text & few_files)),
             "contained_bin": _by(binary_out, single & bin_dev), "edges_bin": _by(binary_out, single & bin_dev),
             "par_simple_edges": _by(ps_files, single & ps_dev)}
    bits = {"chains": chains, "rows_early": single & rows_early, "rows_grouped": single & ~flag["HOST_ROW_SORT"]}
    bits.update(_derived(o, maker, np.where(single, stream, True)))
    full = {k: np.broadcast_to(v, SHAPE) for k, v in {**maker, **bits, **o}.items()}
    return _pack(full, full).reshape(-1), full


def _hex_columns(raw, widths):
    """fixed-width lines of hex numbers as integer columns"""
    a = np.frombuffer(raw, dtype=np.uint8).reshape(-1, sum(widths) + len(widths))
    d = np.where(a >= ord("a"), a - ord("a") + 10, a - ord("0")).astype(np.int64)
    cols, at = [], 0
    for w in widths:
        cols.append(sum(d[:, at + i] << (4 * (w - 1 - i)) for i in range(w)))
        at += w + 1
    return cols


def _unpack(m):
    return {p: (m >> (2 * i)) & 3 for i, p in enumerate(PRODUCTS)}, {b: ((m >> (10 + i)) & 1).astype(bool) for i, b in enumerate(BITS)}


def test_every_routing_variable_is_read_as_a_flag_or_as_a_tri_state():
    build.build_host()
    p = subprocess.run([os.path.join(BIN, "plan_check"), "knobs"], stdout=subprocess.PIPE, text=True)
    assert p.returncode == 0
    got = {l.split()[0]: [int(x) for x in l.split()[1:]] for l in p.stdout.splitlines()}
    want = {"DISCO_" + f: [0, 1, 1] for f in FLAGS + ("HOST_INPUT", "PAR_SIMPLE")}                  # a flag counts when set, whatever its value
    want.update({"DISCO_" + t: [-1, 0, 1] for t in TRIS + ("DIST_DEVICE_INPUT",)})    # unset (the default), "0" off, anything else on
    assert got == want


def test_the_plan_is_the_route_table_for_every_combination_and_every_set_of_demotions():
    build.build_host()
    p = subprocess.run([os.path.join(BIN, "plan_check")], stdout=subprocess.PIPE)
    assert p.returncode == 0
    want, full = _table()
    n = want.size
    (got,) = _hex_columns(p.stdout[:6 * n], [5])
    assert got.shape == want.shape
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(dict(zip(AXES, np.unravel_index(i, SHAPE))), hex(got[i]), hex(want[i])) for i in bad[:5]]
    maker, bits = _unpack(want)
    # a product is None exactly when its flag does not ask for it; under --no-text both text products are None
    f = {k: v.reshape(-1) for k, v in full.items()}
    asked = {"contained_text": ~f["no_text"], "edge_text": ~f["no_text"], "contained_bin": f["binary_out"], "edges_bin": f["binary_out"],
             "par_simple_edges": f["par_simple"] & ~f["mpi_names"]}
    for prod in PRODUCTS:
        assert np.array_equal(maker[prod] != NONE, asked[prod]), prod
    assert not (f["no_text"] & ((maker["contained_text"] != NONE) | (maker["edge_text"] != NONE))).any()
    # the demotions: every plan that occurs under each combination of options, with every subset of its Device products demoted
    opt_index = np.arange(n) // (2 ** len(FLAGS) * 3 ** len(TRIS))
    oi, before, demoted, after = _hex_columns(p.stdout[6 * n:], [2, 5, 2, 5])
    occurring = np.unique(opt_index * (1 << 17) + want)
    assert np.array_equal(np.unique(oi * (1 << 17) + before), occurring)
    mk, bt = _unpack(before)
    device_set = sum((mk[prod] == DEVICE).astype(np.int64) << i for i, prod in enumerate(PRODUCTS))
    assert ((demoted & ~device_set) == 0).all()
    key = (oi * (1 << 17) + before) * 32 + demoted
    assert np.unique(key).size == key.size == sum(1 << bin(int(d)).count("1") for d in device_set[demoted == 0])   # all subsets, each once
    o = _options(*np.unravel_index(oi, (2, 3, 16))[:2], (oi % 16) // 8, (oi % 16) // 4 % 2)
    mk_after = {prod: np.where((demoted >> i) & 1 == 1, HOST, mk[prod]) for i, prod in enumerate(PRODUCTS)}
    bt_after = dict(bt, **_derived(o, mk_after, bt["streamed"]))
    assert np.array_equal(after, _pack(mk_after, bt_after))
    # a demotion never takes the rows or the edges off the host
    _, got_after = _unpack(after)
    assert not (bt["rows_on_host"] & ~got_after["rows_on_host"]).any() and not (bt["edges_on_host"] & ~got_after["edges_on_host"]).any()
    assert (demoted != 0).sum() > 1000
