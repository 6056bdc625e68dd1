"""The host step of the direct build (include/vnr_amd.h, "corrections built straight into bit planes"; csrc/correction_direct.cpp):
from the per-cell pairs {max |q|, sum of nbits} that pass 1 folds to the entries {cell, width} of the flagged cells and to each one's
first group and first plane word.  The pairs are derived in numpy from the blobs of tests/correction_pack_cases.py, the expected
index is tests/correction_index_ref.py's, and the library code runs in a stand-alone program under address / undefined-behaviour
sanitizers.  CPU only; every comparison has tolerance zero.

The crafted blobs hold the most negative code of their width (-128 in a 1-byte cell), which no build stores at that width: the width
rule is on max |q| (<= 127: 1, <= 32767: 2, else 4), so the expected width of such a cell is the rule's, restated here, and the 4-byte
one, whose max |q| is 2^31, is the refusal."""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import correction_index_ref as cir  # noqa: E402
import correction_pack_cases as cases  # noqa: E402
import correction_pack_ref as cpr  # noqa: E402
import error_bound_ref as ebr  # noqa: E402

TYPE_SIZE = {code: np.dtype(dt).itemsize for dt, code in ebr.VALUE_TYPES.items()}


def all_blobs():
    out = [(i, cases.case(*c)["bytes"]) for i, c in zip(cases.IDS, cases.CASES)]
    out += [("many-cells", cases.many_cells()["bytes"])]
    return out + [(f"crafted-{t.__name__}-{e}-w{w}", cases.crafted(t, e, w)[0]) for t, e, w in cases.CRAFTED]


def cell_groups(dims):
    n_cells = int(np.prod([-(-d // 16) for d in dims]))
    return [-(-cpr.cell_voxels(dims, c) // 64) for c in range(n_cells)]


def pairs_of(v1):
    """-> (dims, kind, type size, [[max |q|, sum of nbits]] for every cell of the grid) as pass 1 would fold them: max |q| saturated
    to 32 bits (kind 2: 1 where a voxel differs, so 1 for a flagged cell), nbits summed over the cell's groups; the unflagged cells of
    kind 2 get a nonzero sum, which the plan must not look at"""
    f, cells, payload = cpr.split(v1, b"VNRCORR1")
    dims, kind = f[3:6], f[10]
    ix = cir.index(cpr.pack(v1))
    groups = cell_groups(dims)
    pairs = [[0, 7 + c % 50 if kind == 2 else 0] for c in range(len(groups))]
    at = 0
    for i, (cell, width) in enumerate(cells):
        n = cpr.cell_voxels(dims, cell)
        q = np.frombuffer(payload, cpr.CODE[width], n, at).astype(np.int64)
        at += n * width + (-(n * width) % 16)
        g0 = ix["cell_group0"][i]
        pairs[cell] = [1 if kind == 2 else min(int(np.abs(q).max()), 0xffffffff), int(ix["nbits"][g0:g0 + groups[cell]].sum())]
    return dims, kind, TYPE_SIZE[f[2]], pairs


def rule_width(kind, type_size, m):
    return type_size if kind == 2 else (1 if m <= 127 else (2 if m <= 32767 else 4))


def expected_text(v1, pairs):
    """what tests/correction_direct_harness.cpp prints: the entries by the width rule, the places from correction_index_ref.index"""
    f, cells, _ = cpr.split(v1, b"VNRCORR1")
    dims, kind, type_size = f[3:6], f[10], TYPE_SIZE[f[2]]
    if any(m > 2**31 - 1 for m, _ in pairs):
        return "refused\n"
    ix = cir.index(cpr.pack(v1))
    grid_group0 = np.concatenate([[0], np.cumsum(cell_groups(dims))])
    flagged = [c for c, (m, _) in enumerate(pairs) if m]
    assert flagged == [c for c, _ in cells] == ix["cells"]
    lines = ["cells %d groups %d words %d" % (len(flagged), len(ix["group_word"]), ix["n_words"])]
    lines += ["e %d %d %d %d %d" % (c, rule_width(kind, type_size, pairs[c][0]), grid_group0[c], g, w)
              for c, g, w in zip(flagged, ix["cell_group0"], ix["cell_word0"])]
    return "\n".join(lines) + "\n"


def case_file(path, dims, kind, type_size, pairs):
    with open(path, "w") as f:
        f.write("%d %d %d %d %d %d\n" % (*dims, kind, type_size, len(pairs)))
        f.write("".join("%d %d\n" % (m, n) for m, n in pairs))


def test_the_pairs_cover_every_width_clean_cells_and_the_refusal():
    seen_widths, clean, refused, rewidened = set(), 0, 0, 0
    for name, v1 in all_blobs():
        f, cells, _ = cpr.split(v1, b"VNRCORR1")
        dims, kind, type_size, pairs = pairs_of(v1)
        if any(m > 2**31 - 1 for m, _ in pairs):
            refused += 1
            continue
        widths = [rule_width(kind, type_size, pairs[c][0]) for c, _ in cells]
        if name.startswith("crafted"):
            rewidened += widths != [w for _, w in cells]
        else:
            assert widths == [w for _, w in cells], name              # what a build stores obeys the rule
        seen_widths.update(widths)
        clean += sum(1 for m, _ in pairs if m == 0)
    assert seen_widths == {1, 2, 4, 8} and clean > 0 and refused == 1 and rewidened >= 2


def test_library_plan_equals_numpy_under_sanitizers(tmp_path):
    """csrc/correction_direct.cpp (with the two format files it calls) compiled with -fsanitize=address,undefined into a stand-alone
    program (a CPU build; a subprocess): entries, first groups and first plane words of every blob are the numpy ones; a pair with
    max |q| = 2^31 is refused and gives nothing, one with 2^31 - 1 is a 4-byte cell"""
    texts, paths = [], []

    def add(dims, kind, type_size, pairs, want):
        paths.append(str(tmp_path / f"case{len(paths)}.txt"))
        case_file(paths[-1], dims, kind, type_size, pairs)
        texts.append(want)

    for _, v1 in all_blobs():
        dims, kind, type_size, pairs = pairs_of(v1)
        add(dims, kind, type_size, pairs, expected_text(v1, pairs))
    # the edge of the refusal, on the int32 case of 40 x 24 x 20: its last flagged cell
    v1 = cases.case(np.int32, 1, (40, 24, 20))["bytes"]
    dims, kind, type_size, pairs = pairs_of(v1)
    last = max(c for c, (m, _) in enumerate(pairs) if m)
    edge = [list(p) for p in pairs]
    edge[last][0] = 2**31
    add(dims, kind, type_size, edge, "refused\n")
    edge[last][0] = 2**31 - 1
    want = expected_text(v1, edge)
    assert want.splitlines()[-1].split()[:3] == ["e", str(last), "4"]
    add(dims, kind, type_size, edge, want)
    # no flagged cell at all
    add(dims, kind, type_size, [[0, 0]] * len(pairs), "cells 0 groups 0 words 0\n")

    exe = str(tmp_path / "correction_direct_harness")
    csrc = os.path.join(os.path.dirname(HERE), "instantvnr_amd", "csrc")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                        os.path.join(HERE, "correction_direct_harness.cpp"), os.path.join(csrc, "correction_direct.cpp"),
                        os.path.join(csrc, "correction_packed_format.cpp"), os.path.join(csrc, "correction_format.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    h = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=600)
    assert h.returncode == 0, (h.returncode, h.stdout[-500:], h.stderr[-3000:])
    assert h.stdout == "".join(f"file {i}\n{t}" for i, t in enumerate(texts))
    assert texts.count("refused\n") == 2


def test_the_series_tool_offers_the_direct_build():
    root = os.path.dirname(HERE)
    text = open(os.path.join(root, "tools", "README.md")).read()
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "insitu_series.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    assert "--direct" in text and "--direct" in out.stdout
