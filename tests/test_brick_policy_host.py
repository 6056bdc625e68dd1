"""The inference cache's decisions (csrc/brick_policy.h): which levels a brick image takes within a budget, and when an image is built, kept
and given up.  The library code runs in a stand-alone program (tests/brick_policy_harness.cpp) under the address / undefined-behaviour
sanitizers; what it must answer is restated here in Python from the rules (csrc/brick_policy.h, csrc/grid_levels.h), not taken from the
library.  CPU only; every comparison is exact.

The rules.  Plan: only levels with hashed == 1; not those with resolution > cap + 1 (cap 0: no cap); F <= 2 finest first, F >= 4 coarsest
first; a brick is one 128-byte line of 64 / F entries, 4x4x4 (F = 1), 8x2x2 with 7 useful columns (F = 2: res / 7 + 1 bricks per row, kept in
pad1, and no level of resolution >= 13000), 4x2x2 (F = 4), 2x2x2 (F = 8); a level is skipped when it has >= 2^32 entries, when the running
total + its lines + the spare line exceed the budget, or reach 0xffffffff; brick = running total + 1; bytes = (used + 1) * 128.
Policy: mode 0 never builds; a full image is asked for at the first launch in mode 1, else once more launches than after_now() = base * scale
(64-bit, clamped to 2^32 - 1) have seen unchanged parameters; a small one when nothing is served, the launch holds >= 2^20 samples, F <= 2
and there is a small budget.  A parameter change drops what is served; of a full image that served < 64 launches it doubles the scale (up
to 65536), of one that served more it resets it; a small image never moves it."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "instantvnr_amd", "csrc")
BIG = 1 << 20


# ------------------------------------------------------------------------------------------------ the rules, restated
def layout(L, base, scale, log2T):
    """grid_make_layout for a Hash grid: [(resolution, size, offset, hashed)]"""
    out, offset = [], 0
    for l in range(L):
        res = int(-(-(scale ** l * base - 1.0) // 1)) + 1
        n = min(res ** 3, 0xffffffff // 2)
        n = min(-(-n // 8) * 8, 1 << log2T)
        stride, dims = 1, 0
        while dims < 3 and stride <= n:
            stride, dims = stride * res, dims + 1
        out.append((res, n, offset, 1 if n < stride else 0))
        offset += n
    return out


LOG_SHAPE = {1: (2, 2, 2), 2: (3, 1, 1), 4: (2, 1, 1), 8: (1, 1, 1)}


def plan(levels, F, cap, budget_lines):
    lx, ly, lz = LOG_SHAPE[F]
    assert (1 << (lx + ly + lz)) * F * 2 == 128
    rows = {l: [0, 0, 0, 0, 0, 0] for l in range(len(levels))}   # brick pad1 lines nbx nby nbz
    used, mask = 0, 0
    order = range(len(levels) - 1, -1, -1) if F <= 2 else range(len(levels))
    for l in order:
        res, size, offset, hashed = levels[l]
        if hashed != 1 or (cap and res > cap + 1) or (F == 2 and res >= 13000):
            continue
        nb = [res // 7 + 1 if F == 2 else (res >> lx) + 1, (res >> ly) + 1, (res >> lz) + 1]
        lines = nb[0] * nb[1] * nb[2]
        if lines * (64 // F) >= 2 ** 32 or used + lines + 1 > budget_lines or used + lines + 1 >= 0xffffffff:
            continue
        rows[l] = [used + 1, nb[0] if F == 2 else 0, lines] + nb
        used += lines
        mask |= 1 << l
    return used, mask, rows


def plan_script(levels, F, cap, budget_lines):
    return "plan %d %d %d %d\n" % (F, cap, budget_lines, len(levels)) + "".join("%d %d %d %d\n" % lv for lv in levels)


def plan_text(levels, F, cap, budget_lines):
    used, mask, rows = plan(levels, F, cap, budget_lines)
    head = "plan used %d mask %d bytes %d empty %d epl %d\n" % (used, mask, (used + 1) * 128, used == 0, 64 // F)
    return head + "".join("  %d %d %d %d %d %d %d\n" % (l, *rows[l]) for l in range(len(levels)))


class Policy:
    """the transitions, and the text the harness prints after each"""

    def __init__(self, env_mode, after_base, small_budget):
        self.env_mode, self.base, self.small_budget = env_mode, after_base, small_budget
        self.tier = self.stable = self.served = self.builds = self.small_builds = 0
        self.scale, self.full_refused, self.small_refused, self.mode = 1, False, False, -1
        self.script, self.text = [], []
        self.say("policy %d %d %d" % (env_mode, after_base, small_budget), "policy")

    def after_now(self):
        return min(self.base * self.scale, 2 ** 32 - 1)

    def say(self, op, head):
        self.script.append(op)
        self.text.append("%s tier %d stable %d served %d scale %d after %d builds %d small_builds %d refused %d %d mode %d" % (
            head, self.tier, self.stable, self.served, self.scale, self.after_now(), self.builds, self.small_builds, self.full_refused,
            self.small_refused, self.mode))

    def resolved(self):
        return self.mode if self.mode >= 0 else self.env_mode

    def launch(self, n_max=64, F=2, outcome="ok"):
        ask = 0
        if self.resolved() != 0 and not self.full_refused and self.tier != 2:
            self.stable = min(self.stable + 1, 2 ** 32 - 1)
            if self.resolved() == 1 or self.stable > self.after_now():
                ask = 2
            elif self.tier == 0 and not self.small_refused and n_max >= BIG and self.small_budget > 0 and F <= 2:
                ask = 1
        if ask and outcome == "empty":          # that tier's refusal; what is served stays
            if ask == 2:
                self.full_refused = True
            else:
                self.small_refused = True
        elif ask:
            self.tier = ask
            if ask == 2:
                self.served = 0
            if outcome == "ok":                  # (shortcut: the small image is promoted, nothing was built)
                if ask == 2:
                    self.builds += 1
                else:
                    self.small_builds += 1
        serve = self.resolved() != 0 and self.tier != 0
        if serve:
            self.served = min(self.served + 1, 2 ** 32 - 1)
        self.say("launch %d %d %s" % (n_max, F, outcome), "launch ask %d serve %d" % (ask, serve))
        return ask

    def params(self):
        if self.tier == 2:
            self.scale = min(self.scale * 2, 65536) if self.served < 64 else 1
        self.tier = self.stable = self.served = 0
        self.say("params", "params")

    def set_mode(self, m):
        self.mode = -1 if m < 0 else min(m, 1)
        self.full_refused = self.small_refused = False
        self.stable = 0
        self.say("mode %d" % m, "mode")

    def budget(self):
        self.full_refused = self.small_refused = False
        self.stable = 0
        self.say("budget", "budget")

    def released(self):
        self.tier = self.stable = 0
        self.say("released", "released")

    def sync(self, held, new):
        self.script.append("sync %d %d" % (held, new))
        self.text.append("sync %d" % (held != 0 and (held != new or self.tier != 0)))


# ------------------------------------------------------------------------------------------------ the cases
LEVELS = layout(6, 4, 2.0, 10)


def plan_cases():
    """[(levels, F, cap, budget_lines)]"""
    ample = 1 << 30
    far = [(13000, 1 << 19, 0, 1), (12999, 1 << 19, 1 << 19, 1), (100, 1 << 19, 1 << 20, 1)]
    huge = [(1 << 12, 1 << 19, 0, 1), (100, 1 << 19, 1 << 19, 1)]   # 4097 x 2049 x 2049 bricks of 8 entries: >= 2^32 entries
    return [(LEVELS, 8, 0, 4_800_000 // 128), (LEVELS, 2, 0, 1_450_000 // 128), (LEVELS, 1, 0, ample), (LEVELS, 4, 0, ample), (LEVELS, 2, 0, ample),
            (LEVELS, 8, 0, ample), (LEVELS, 2, 64, ample), (LEVELS, 8, 63, ample), (LEVELS, 2, 0, 0), (LEVELS, 8, 0, 1), (far, 2, 0, ample),
            (far, 1, 0, ample), (huge, 8, 0, 1 << 40), (LEVELS, 1, 0, 2 ** 32 + 10)]


def test_the_restated_plan_rule_gives_the_hand_checked_cases():
    assert [lv[0] for lv in LEVELS] == [4, 8, 16, 32, 64, 128] and [lv[3] for lv in LEVELS] == [0, 0, 1, 1, 1, 1]
    used, mask, rows = plan(LEVELS, 8, 0, 4_800_000 // 128)
    assert 4_800_000 // 128 == 37_500 and (rows[2][2], rows[3][2]) == (729, 4913) and mask == 0b1100 and 35_937 + used + 1 > 37_500
    used, mask, rows = plan(LEVELS, 2, 0, 1_450_000 // 128)
    assert 1_450_000 // 128 == 11_328 and (rows[4][2], rows[2][2]) == (10_890, 243) and mask == 0b10100
    assert plan(LEVELS, 2, 0, 1 << 30)[2][5][2] == 80_275 and plan(LEVELS, 2, 0, 1 << 30)[2][3][2] == 1_445
    seen = set()
    for levels, F, cap, budget in plan_cases():
        used, mask, rows = plan(levels, F, cap, budget)
        if used:
            assert (used + 1) * 128 <= budget * 128                                     # bytes() <= budget
        at = 1
        for l in (sorted(rows, reverse=True) if F <= 2 else sorted(rows)):              # brick offsets: the running sum + 1
            if rows[l][2]:
                assert rows[l][0] == at and rows[l][1] == (levels[l][0] // 7 + 1 if F == 2 else 0)
                at += rows[l][2]
            else:
                assert rows[l][:2] == [0, 0]
        seen.add((F, used == 0, mask))
    assert (2, True, 0) in seen and (8, True, 0) in seen                                # the empty plans
    assert plan(LEVELS, 2, 64, 1 << 30)[1] == 0b011100 and plan(LEVELS, 8, 63, 1 << 30)[1] == 0b011100   # the cap takes the finest level
    # res 13000 is skipped (and, a level that fine having >= 2^32 image entries at any F, so is 12999)
    assert plan(plan_cases()[10][0], 2, 0, 1 << 30)[1] == 0b100 and plan(plan_cases()[11][0], 1, 0, 1 << 30)[1] == 0b100
    assert plan(plan_cases()[12][0], 8, 0, 1 << 40)[1] == 0b10


def policy_sequences():
    out = []
    # base 24: the first full build on the 25th stable launch; dropped young: 48; an image that served >= 64 launches: back to 24
    p = Policy(-1, 24, 0.75 * 2 ** 30)
    asks = [p.launch(64, 2) for _ in range(25)]
    assert asks == [0] * 24 + [2] and p.builds == 1 and p.tier == 2
    for _ in range(5):
        p.launch(5000, 2)
    p.params()
    assert p.after_now() == 48 and p.tier == 0
    asks = [p.launch(64, 2) for _ in range(49)]
    assert asks == [0] * 48 + [2] and p.builds == 2
    for _ in range(63):
        p.launch(64, 2)
    assert p.served == 64
    p.params()
    assert p.after_now() == 24
    out.append(p)
    # small tier: four cycles of change + frame -> 4 small builds, no full one, the threshold does not move; then one full build
    p = Policy(-1, 24, 0.75 * 2 ** 30)
    for _ in range(4):
        p.params()
        assert p.launch(BIG, 2) == 1
        for _ in range(11):
            assert p.launch(BIG, 2) == 0
    assert (p.small_builds, p.builds, p.after_now(), p.tier) == (4, 0, 24, 1)
    for _ in range(30):
        p.launch(BIG, 2)
    assert (p.small_builds, p.builds, p.tier) == (4, 1, 2)
    out.append(p)
    # never the small tier: a launch below 2^20, F = 4, no small budget, or refused before
    p = Policy(-1, 24, 0.75 * 2 ** 30)
    assert [p.launch(BIG - 1, 2), p.launch(BIG, 4), p.launch(BIG, 8)] == [0, 0, 0]
    assert p.launch(BIG, 1, "empty") == 1 and p.small_refused and not p.full_refused
    assert p.launch(BIG, 1) == 0
    out.append(p)
    p = Policy(-1, 24, 0.0)
    assert p.launch(BIG, 2) == 0
    out.append(p)
    # modes: 0 never builds (set or from the environment), 1 asks at the first launch; a set mode overrides the environment's
    p = Policy(0, 0, 0.75 * 2 ** 30)
    assert [p.launch(BIG, 2) for _ in range(3)] == [0, 0, 0] and p.stable == 0
    p.set_mode(1)
    assert p.launch(64, 8) == 2 and p.tier == 2
    p.set_mode(0)
    p.released()            # (what the cache does with a served image in mode 0)
    assert p.launch(64, 8) == 0 and p.tier == 0
    p.set_mode(-1)
    assert p.launch(64, 8) == 0
    out.append(p)
    p = Policy(1, 24, 0.75 * 2 ** 30)
    assert p.launch(64, 2) == 2
    p.budget()
    p.released()
    assert p.launch(64, 2, "empty") == 2 and p.full_refused and p.tier == 0
    assert p.launch(64, 2) == 0               # latched ...
    p.budget()
    assert p.launch(64, 2) == 2               # ... until the budget or the mode changes
    out.append(p)
    # an empty full plan while a small image is served: tier 1 keeps serving, only the full refusal is latched
    p = Policy(-1, 2, 0.75 * 2 ** 30)
    assert p.launch(BIG, 2) == 1
    p.launch(BIG, 2)
    assert p.launch(BIG, 2, "empty") == 2
    assert p.tier == 1 and p.full_refused and not p.small_refused
    served = p.served
    assert p.launch(BIG, 2) == 0 and p.served == served + 1 and p.text[-1].startswith("launch ask 0 serve 1")
    out.append(p)
    # the shortcut: the small image is the full one -> tier 2, build counter unchanged
    p = Policy(-1, 2, 0.75 * 2 ** 30)
    p.launch(BIG, 2)
    p.launch(BIG, 2)
    assert p.launch(BIG, 2, "shortcut") == 2 and (p.tier, p.builds, p.small_builds) == (2, 0, 1)
    out.append(p)
    # 65536 x 65536 is 2^32 - 1, not 0
    p = Policy(1, 65536, 0.0)
    for _ in range(17):
        p.launch(64, 8)
        p.params()
    assert p.scale == 65536 and p.after_now() == 2 ** 32 - 1
    out.append(p)
    # overwriting: the device is idled whenever the replaced image is served, equal size or not; an unserved buffer only when it is freed
    p = Policy(-1, 24, 0.75 * 2 ** 30)
    p.sync(0, 4096)
    p.launch(BIG, 2)
    p.sync(4096, 4096)
    p.sync(4096, 8192)
    p.params()
    p.sync(4096, 4096)
    p.sync(4096, 8192)
    assert [t for t in p.text if t.startswith("sync")] == ["sync 0", "sync 1", "sync 1", "sync 0", "sync 1"]
    out.append(p)
    return out


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("brick_policy") / "brick_policy_harness")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + CSRC,
                        os.path.join(HERE, "brick_policy_harness.cpp"), os.path.join(CSRC, "brick_policy.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    return exe


def run(exe, tmp_path, script):
    path = str(tmp_path / "script.txt")
    with open(path, "w") as f:
        f.write(script)
    h = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
    assert h.returncode == 0, (h.returncode, h.stdout[-500:], h.stderr[-3000:])
    return h.stdout


def test_library_plan_equals_the_restated_rule_under_sanitizers(harness, tmp_path):
    cases = plan_cases()
    got = run(harness, tmp_path, "".join(plan_script(*c) for c in cases))
    assert got == "".join(plan_text(*c) for c in cases)


def test_library_policy_equals_the_restated_transitions_under_sanitizers(harness, tmp_path):
    for i, p in enumerate(policy_sequences()):
        got = run(harness, tmp_path, "\n".join(p.script) + "\n")
        assert got.splitlines() == p.text, i


def test_the_policy_header_needs_no_hip():
    """brick_policy.h and what it includes compile without the HIP headers (the harness is built by g++ with nothing but csrc/ on its path)"""
    for name in ("brick_policy.h", "brick_policy.cpp", "grid_levels.h"):
        text = open(os.path.join(CSRC, name)).read()
        assert "common.h" not in text and "hip/" not in text, name
