"""numpy restatement of the index over a packed correction (include/vnr_amd.h, "resident form"; correction_plane_index of
csrc/correction_packed_format.cpp) on top of correction_pack_ref.py: where the plane words of every group start, and code_at(),
which reads a code out of the planes through that index the way the apply kernel of the packed resident form does."""
import numpy as np

import correction_pack_ref as cpr

ONE = np.uint64(1)


def index(packed):
    """-> dict: per flagged cell cell_group0 (groups in front of it) and cell_word0 (plane words in front of it), per group
    group_word (the plane words of its cell in front of it) and nbits, n_words, and the planes as uint64 words"""
    f, cells, payload = cpr.split(packed, b"VNRCORP1")
    dims = f[3:6]
    cell_group0, cell_word0, group_word, nbits = [], [], [], []
    g = words = 0
    for cell, _ in cells:
        cell_group0.append(g)
        cell_word0.append(words)
        in_cell = 0
        for _ in range(-(-cpr.cell_voxels(dims, cell) // 64)):
            group_word.append(in_cell)
            nbits.append(payload[g])
            in_cell += payload[g]
            g += 1
        words += in_cell
    table_bytes = g + (-g % 8)
    assert len(payload) == table_bytes + 8 * words
    assert all(w <= 63 * 64 for w in group_word)
    return {"cells": [c for c, _ in cells], "kind": f[10], "cell_group0": cell_group0, "cell_word0": cell_word0,
            "group_word": np.array(group_word, np.int64), "nbits": np.array(nbits, np.int64), "n_words": words,
            "planes": np.frombuffer(payload, "<u8", words, table_bytes).astype(np.uint64)}


def code_at(ix, i, li):
    """the code of voxel li (an index, or an array of them) of flagged cell number i: voxel -> group li // 64 and lane li % 64, nbits
    and the first word from the index, z = sum_b ((planes[word0 + b] >> lane) & 1) << b.  -> int64, the signed q = (z >> 1) ^ -(z & 1)
    of kinds 0 and 1; uint64, the stored bit pattern z, of kind 2"""
    li = np.asarray(li, np.int64)
    at = np.atleast_1d(li)
    group, lane = ix["cell_group0"][i] + at // 64, (at % 64).astype(np.uint64)
    word0, nbits = ix["cell_word0"][i] + ix["group_word"][group], ix["nbits"][group]
    z = np.zeros(at.shape, np.uint64)
    for b in range(int(nbits.max(initial=0))):              # (nbits == 0: no plane word is read)
        m = nbits > b
        z[m] |= ((ix["planes"][word0[m] + b] >> lane[m]) & ONE) << np.uint64(b)
    out = z if ix["kind"] == 2 else (z >> ONE).view(np.int64) ^ -(z & ONE).view(np.int64)
    return out if li.ndim else out[0]


def index_text(ix):
    """the index as tests/correction_index_harness.cpp prints it"""
    lines = ["cells %d groups %d words %d" % (len(ix["cells"]), len(ix["group_word"]), ix["n_words"])]
    lines += ["c %d %d" % (g, w) for g, w in zip(ix["cell_group0"], ix["cell_word0"])]
    lines += ["g %d" % w for w in ix["group_word"]]
    return "\n".join(lines) + "\n"
