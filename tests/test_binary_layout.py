"""CPU: the records of the binary side output as include/disco_hip.h declares them (disco_bin_edge / disco_bin_contained, what the device
writes) have the layout disco_amd/edgefile.py reads: a C99 compiler's sizeof / offsetof of every field against the numpy dtypes."""
import os
import subprocess

from disco_amd import edgefile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (C field, numpy field) in declaration order
EDGE_FIELDS = [("src", "src"), ("dst", "dst"), ("orient", "orient"), ("offset", "offset"), ("len_src", "len_src"), ("len_dst", "len_dst"), ("file", "file"),
               ("flag", "flag"), ("substitutions", "substitutions")]
CONTAINED_FIELDS = [("contained", "contained"), ("super", "super"), ("orient", "orient"), ("len2", "len2"), ("len1", "len1"), ("start", "start"), ("file", "file"),
                    ("pad0", "pad0"), ("pad1", "pad1")]


def _c_layout(tmp_path):
    def prints(typ, fields):
        return "".join(f'    printf("%zu %zu\\n", offsetof({typ}, {c}), sizeof((({typ} *)0)->{c}));\n' for c, _ in fields)

    src = tmp_path / "binlay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "disco_hip.h"\nint main(void)\n{\n'
                   '    printf("%zu %zu\\n", sizeof(disco_bin_edge), sizeof(disco_bin_contained));\n'
                   + prints("disco_bin_edge", EDGE_FIELDS) + prints("disco_bin_contained", CONTAINED_FIELDS) + "    return 0;\n}\n")
    exe = tmp_path / "binlay"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    rows = [tuple(int(x) for x in line.split()) for line in subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()]
    return rows[0], rows[1:1 + len(EDGE_FIELDS)], rows[1 + len(EDGE_FIELDS):]


def test_the_header_s_records_have_the_layout_edgefile_reads(tmp_path):
    sizes, edge, contained = _c_layout(tmp_path)
    assert sizes == (edgefile.EDGE.itemsize, edgefile.CONTAINED.itemsize) == (40, 40)
    for got, fields, dt in ((edge, EDGE_FIELDS, edgefile.EDGE), (contained, CONTAINED_FIELDS, edgefile.CONTAINED)):
        assert [n for _, n in fields] == list(dt.names)          # every field, in order
        want = [(dt.fields[n][1], dt.fields[n][0].itemsize) for _, n in fields]
        assert got == want, (got, want)
        assert sum(s for _, s in want) == dt.itemsize            # no padding between or behind the fields: every byte belongs to one
