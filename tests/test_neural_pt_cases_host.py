"""Every model of tests/neural_pt_cases.py gives the oracle's path tracer something to show: conditions on the reference alone (the oracle's
path tracer fed by the oracle's network), which keep the GPU comparisons that use these models from comparing black frames."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neural_pt_cases as npc  # noqa: E402


@pytest.fixture(scope="module")
def host_scene(oracle):
    return npc.HostScene(oracle)


def test_the_case_table_reaches_every_in_shader_encoding_shape_and_width():
    """(F, padded encoded width) of VNR_IN_SHADER_SHAPES (csrc/in_shader.h), all nine, and the four network widths"""
    shapes = {(c["F"], (c["L"] * c["F"] + 15) // 16 * 16) for c in npc.CASES.values()}
    assert shapes == {(1, 16), (1, 32), (2, 16), (2, 32), (2, 64), (4, 32), (4, 64), (8, 64), (8, 128)}
    assert {c["W"] for c in npc.CASES.values()} == {16, 32, 64, 128}
    for name in ("f1-k32", "f2-k64", "f4-k64", "f8-k128"):     # the many-level cases keep their finest level below 512
        c = npc.CASES[name]
        assert c["base"] * c["pls"] ** (c["L"] - 1) < 512


@pytest.mark.parametrize("name", sorted(npc.CASES))
def test_every_case_is_lit_and_its_value_varies_in_space(oracle, host_scene, name):
    case = npc.CASES[name]
    params = npc.parameters(oracle, case)
    net = npc.oracle_network(oracle, case, params)
    values = net(np.random.default_rng(0).uniform(0, 1, (4000, 3)).astype(np.float32))
    assert np.isfinite(values).all()
    frame, _, stats = oracle.render_pathtracing(host_scene.holder(oracle, mode=14, frame_index=1), net)
    lit, spread = npc.lit_share(frame), npc.value_spread(values)
    print(f"\n{name}: lit {lit:.3f}, q95 - q05 {spread:.3f}, {stats['n_samples']} samples")
    assert lit >= npc.MIN_LIT, (name, lit)
    assert spread >= npc.MIN_VALUE_SPREAD, (name, spread)
