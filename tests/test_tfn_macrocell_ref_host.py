"""tests/tfn_macrocell_ref.py (numpy, from the definitions) against the C oracle, bit for bit, on every input set that
tests/test_gpu_tfn_macrocell.py then puts to the library; and each of five deliberately broken variants of the restatement must differ from
the oracle on those same inputs, so that a kernel with that mistake could not pass there either.  No GPU."""
import numpy as np
import pytest

import tfn_macrocell_ref as ref

TABLE_PAIRS = [(n, n) for n in ref.ALPHA_LENGTHS] + [(1536, 1), (300, 4096), (1, 17)]


def holder(oracle, colors, alphas, window):
    return oracle.TfnHolder(colors, alphas, *ref.tfn_window(*window)[:2])


def lookup_cases():
    for n_colors, n_alphas in TABLE_PAIRS:
        for window in ref.WINDOWS:
            yield ref.color_table(n_colors), ref.alpha_table(n_alphas), window, ref.lookup_values(window, max(n_colors, n_alphas))


def range_cases(oracle):
    return {"implicit": oracle.macrocell_compute_implicit(ref.ragged_volume()), "online": ref.online_range()}


def opacity_cases(oracle):
    for name, vr in range_cases(oracle).items():
        for n in ref.ALPHA_LENGTHS:
            for alphas in ref.bound_tables(n).values():
                for window in ref.WINDOWS:
                    yield name, vr, alphas, window


def update_cases():
    for dims in ref.VOLUMES:
        for n in ref.BATCH_SIZES:
            yield dims, ref.batch(dims, n)


def test_the_window_is_the_transfer_function_s_range_clamped_to_the_data_s():
    for (lo, hi), want in zip(ref.WINDOWS, [(0.0, 1.0), (0.25, 0.7), (0.5, 0.5 + 2.0 ** -20), (0.0, 0.4), (0.6, 1.0)]):
        got = ref.tfn_window(lo, hi)
        assert got[0] == np.float32(want[0]) and got[1] == np.float32(want[1])
        assert got[2] == np.float32(1.0) / (np.float32(want[1]) - np.float32(want[0])) and np.isfinite(got[2])
        assert all(isinstance(v, np.float32) for v in got)
    assert ref.tfn_window(0.5, 0.5 + 2.0 ** -20)[2] == np.float32(2.0 ** 20)
    assert ref.tfn_window(-3.0, 9.0, -1.0, 2.0)[:2] == (np.float32(-1.0), np.float32(2.0))


def test_lookup_equals_the_oracle(oracle):
    for colors, alphas, window, values in lookup_cases():
        want = oracle.tfn_sample(holder(oracle, colors, alphas, window), values)
        got = ref.tfn_lookup(colors, alphas, ref.tfn_window(*window), values)
        assert np.array_equal(got, want), (colors.shape[0], alphas.shape[0], window)


def test_max_opacity_equals_the_oracle(oracle):
    ranges = range_cases(oracle)
    # the two value ranges are what they are meant to be: every cell of the dense volume seen, a layer of the online one not
    assert (ranges["implicit"][..., 1] > 0).all() and ranges["implicit"].shape == (4, 3, 2, 2)
    unseen = (ranges["online"] == 0).all(axis=-1)
    assert unseen[3].all() and not unseen[:3].any(), unseen
    some_zero = some_positive = False
    for name, vr, alphas, window in opacity_cases(oracle):
        want = oracle.macrocell_max_opacity(holder(oracle, ref.color_table(2), alphas, window), vr.copy())
        got = ref.max_opacity(alphas, ref.tfn_window(*window), vr)
        assert np.array_equal(got, want), (name, alphas.shape[0], window)
        some_zero |= bool((want == 0).any())
        some_positive |= bool((want > 0).any())
    assert some_zero and some_positive


def test_explicit_update_equals_the_oracle(oracle):
    for dims, (coords, values) in update_cases():
        want = oracle.macrocell_update_explicit(ref.empty_range(dims), dims, coords, values)
        got = ref.explicit_update(ref.empty_range(dims), dims, coords, values)
        assert np.array_equal(got, want), (dims, coords.shape[0])
        # merged into a macrocell that holds something already, values of both signs in both channels
        again = ref.batch(dims, 257, seed=3)
        want2 = oracle.macrocell_update_explicit(want.copy(), dims, *again)
        assert np.array_equal(ref.explicit_update(got, dims, *again), want2), (dims, coords.shape[0])


def test_training_batches_and_frame_tables_equal_the_oracle_too(oracle):
    """the other inputs of the GPU tests: a training batch of the sampler's pcg32 stream and one of a sampling table's draws (65 536 samples
    in [0, 1), values of the ground truth), and the frame tests' ramp tables over the 48^3 volume's macrocell"""
    import guided_sampling_ref as gref
    from instantvnr_amd import synthetic as syn
    dims = ref.VOLUMES[0]
    vox = np.random.default_rng(3).uniform(0.0, 1.0, dims[::-1]).astype(np.float32)
    w = np.zeros(ref.cell_dims(dims)[::-1], np.float32)
    w[:2, :2, :] = 0.5
    for coords in (gref.uniform_coords(1 << 16, 0, 4242, 5), gref.draw(gref.table(w, 0.0), dims, 1 << 16, 0, 99, 11)[0]):
        values = gref.values(vox, coords)
        start = ref.online_range()
        want = oracle.macrocell_update_explicit(start.copy(), dims, coords, values)
        assert np.array_equal(ref.explicit_update(start, dims, coords, values), want)
    vr = oracle.macrocell_compute_implicit(syn.analytic_volume(48))
    for n in (1, 256, 1228, 1229, 4096):
        alphas = syn.tfn_ramp_with_bumps(n=n)[1] if n > 1 else np.array([0.3], np.float32)
        for window in ref.WINDOWS:
            want = oracle.macrocell_max_opacity(holder(oracle, ref.color_table(2), alphas, window), vr.copy())
            assert np.array_equal(ref.max_opacity(alphas, ref.tfn_window(*window), vr), want), (n, window)


def test_the_batches_hold_what_they_are_meant_to():
    for dims, (coords, values) in update_cases():
        n = coords.shape[0]
        assert coords.dtype == values.dtype == np.float32 and coords.shape == (n, 3) and values.shape == (n,)
        assert not np.isnan(coords).any() and not np.isnan(values).any()
        if n < 5000:
            continue
        for a in range(3):
            d = dims[a]
            lattice = np.arange(d + 1, dtype=np.float32) / np.float32(d)
            on = np.isin(coords[:, a], lattice)
            assert on.sum() >= 1000
            assert set(np.round(coords[on, a] * d).astype(int)) >= set(range(0, d + 1, 16))   # every cell face of the axis
        assert (coords < 0).any() and (coords > 1).any() and (np.abs(coords) == np.float32(1e30)).sum() == 2
        assert values.min() < -1.5 and values.max() > 2.5
        for v in (0.0, 1.0, -1.0):
            assert (values == np.float32(v)).any()
        assert (np.signbit(values) & (values == 0)).any()
        assert ((values - 1 < 0) & (values + 1 > 0)).any() and (values + 1 < 0).any() and (values - 1 > 0).any()


def _caught(fault, oracle):
    """in how many of the shared inputs the broken variant differs from the oracle, per function"""
    hits = {"lookup": 0, "max_opacity": 0, "update": 0}
    if fault in ("no_window_clamp", "len_for_len_minus_one"):
        for colors, alphas, window, values in lookup_cases():
            want = oracle.tfn_sample(holder(oracle, colors, alphas, window), values)
            hits["lookup"] += not np.array_equal(ref.tfn_lookup(colors, alphas, ref.tfn_window(*window), values, fault=fault), want)
    if fault in ("no_window_clamp", "len_for_len_minus_one", "il_without_minus_one"):
        for _, vr, alphas, window in opacity_cases(oracle):
            want = oracle.macrocell_max_opacity(holder(oracle, ref.color_table(2), alphas, window), vr.copy())
            hits["max_opacity"] += not np.array_equal(ref.max_opacity(alphas, ref.tfn_window(*window), vr, fault=fault), want)
    if fault in ("no_plus_apron", "negative_channels_swapped"):
        for dims, (coords, values) in update_cases():
            want = oracle.macrocell_update_explicit(ref.empty_range(dims), dims, coords, values)
            hits["update"] += not np.array_equal(ref.explicit_update(ref.empty_range(dims), dims, coords, values, fault=fault), want)
    return hits


@pytest.mark.parametrize("fault", ref.FAULTS)
def test_a_broken_restatement_differs_from_the_oracle_on_the_shared_inputs(oracle, fault):
    """if one of these passes unnoticed the inputs are too weak: fix the inputs"""
    hits = _caught(fault, oracle)
    print(f"\n{fault}: differs from the oracle in {hits}")
    expect = {"no_plus_apron": ["update"], "negative_channels_swapped": ["update"], "il_without_minus_one": ["max_opacity"],
              "no_window_clamp": ["max_opacity"], "len_for_len_minus_one": ["lookup", "max_opacity"]}[fault]
    for what in expect:
        assert hits[what] > 0, (fault, what, hits)
    if fault in ("no_plus_apron", "negative_channels_swapped"):
        # every batch but the single sample must catch these on its own, on every volume that has a second cell along y (the axis the variant
        # drops the apron on; a single cell has no neighbour to miss)
        for dims, (coords, values) in update_cases():
            if coords.shape[0] < 255 or (fault == "no_plus_apron" and ref.cell_dims(dims)[1] < 2):
                continue
            want = oracle.macrocell_update_explicit(ref.empty_range(dims), dims, coords, values)
            assert not np.array_equal(ref.explicit_update(ref.empty_range(dims), dims, coords, values, fault=fault), want), (fault, dims, coords.shape[0])
