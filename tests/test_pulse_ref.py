"""CPU: tests/pulse_ref.py pinned.  Its reference arithmetic is oracle.goofer_ref.pulse_train bit for bit on every case and the
golden pulse trains to 5e-6; the two conditions of its bound hold (the reference arithmetic, and the documented table placed by
the reference's onsets, stay inside it on every case); every case has the properties that make it reach its path; and ten planted
faults of the device each fall outside the bound on a named case.  Printed with -s: the worst error / bound and the largest
tabulation term t per batch, and per fault whether the 5e-6 absolute rule on the inputs of tests/test_gpu_kernels.py's pulse
tests would have seen it (docs/HISTORY.md carries both tables)."""
import functools

import numpy as np
import pytest

import pulse_ref as P
from conftest import golden
from oracle import goofer_ref as R

F32, F64 = np.float32, np.float64
BATCHES = [(sr, name) for sr in P.RATES for name in P.cases(sr)]


def test_the_case_list_is_the_issue_s():
    assert [n for sr, n in BATCHES if sr == 44100] == ["a", "b", "c", "d11000", "d11025", "d13230", "d21000", "e", "f", "g0", "g1", "g2",
                                                      "g3"]
    assert [(sr, n) for sr, n in BATCHES if sr != 44100] == [(22050, "c"), (48000, "c"), (96000, "b"), (96000, "c")]


@pytest.mark.parametrize("sr,name", BATCHES)
def test_reference_arithmetic_is_the_oracle_s_bit_for_bit(sr, name):
    b = P.cases(sr)[name]
    for k, f in enumerate(b["f0s"]):
        ref, oi, ot = R.pulse_train(f, sr, *b["model"], return_onsets=True)
        got = P.train(f, sr, *b["model"], exact=False)
        assert got["pulse"].dtype == F32 and np.array_equal(P.bits(got["pulse"]), P.bits(ref)), b["names"][k]
        assert np.array_equal(got["oi"], oi) and np.array_equal(got["ot"], ot), b["names"][k]
        assert P.train(f, sr, *b["model"], exact=True)["pulse"].dtype == F64


def test_reference_arithmetic_against_the_golden_pulse_trains():
    g = golden("pulse_train")
    for k in g["names"]:
        assert np.max(np.abs(P.train(g["f0_" + k], 44100)["pulse"] - g["pulse_" + k])) < 5e-6, k
    assert np.max(np.abs(P.train(g["f0_sr96"], 96000)["pulse"] - g["pulse_sr96"])) < 5e-6
    g = golden("pulse_train_lf")
    assert [tuple(float(v) for v in m) for m in g["models"]] == list(P.LF_MODELS + (P.DEFAULT,))
    for m, model in enumerate(g["models"]):
        for k in g["names"]:
            assert np.max(np.abs(P.train(g["f0_" + k], int(g["sr"]), *model)["pulse"] - g["pulse_%s_%d" % (k, m)])) < 5e-6, (k, m)


@pytest.mark.parametrize("sr,name", BATCHES)
def test_the_two_conditions_of_the_bound(sr, name):
    b, tr = P.cases(sr)[name], P.truth(sr, name)
    ref = P.judge(np.concatenate([t["pulse32"] for t in tr]), tr)
    tab = P.judge(P.device_model(b["f0s"], sr, b["model"]), tr)
    cov = [t for t in tr if (t["A"] > 0).any()]
    c = max(float(P.c_of(t)[t["A"] > 0].max()) for t in cov) if cov else 0.0
    tt = max(float((P.c_of(t) - (t["C"] + 2.0) * (1.0 + 2.0 ** -20))[t["A"] > 0].max()) for t in cov) if cov else 0.0
    print("BOUND %6d %-7s reference arithmetic %.3f, table rows at the reference's onsets %.3f of the bound; largest c %.3f, largest t %.3f"
          % (sr, name, ref["worst"], tab["worst"], c, tt))
    assert ref["ok"], ("the reference arithmetic", ref)
    assert tab["ok"], ("table_row placed by the reference's onsets", tab)
    assert np.isfinite(c)


def _tc_is_on_the_grid(T0, model):
    Ra, _, Rk = model
    tc = (Ra + Rk * (1.0 - Ra)) * T0
    return Rk < 1.0 and abs(tc - round(tc)) < 1e-9


@pytest.mark.parametrize("sr,name", BATCHES)
def test_every_batch_stays_inside_what_the_device_allots(sr, name):
    b, tr = P.cases(sr)[name], P.truth(sr, name)
    assert sum(len(f) for f in b["f0s"]) < 200000
    for f, t in zip(b["f0s"], tr):
        assert t["oi"].size <= t["n"] // 2 + 16                  # its onset slots
        assert np.all(f < sr / 2) and np.all(f >= 0)
        assert np.all((t["ot"] >= 3) & (t["ot"] <= 8192))
        assert not any(_tc_is_on_the_grid(int(v), b["model"]) for v in np.unique(t["ot"]))   # (the bound's blind spot)


def test_a_one_table_row_each():
    b, tr = P.cases(44100)["a"], P.truth(44100, "a")
    assert len(tr) == len(P.A_T0) == 18
    for T0, f, t in zip(P.A_T0, b["f0s"], tr):
        i = int(t["oi"][0])
        assert t["oi"].size == 1 and t["ot"][0] == T0 and t["n"] == i + T0 + 8
        assert f[i] == F32(44100.0 / T0) and not f[i + 1:].any()
        assert np.all(t["C"][i:i + T0] == 1) and not t["C"][:i].any() and not t["C"][i + T0:].any()
    assert max(t["n"] for t in tr) == 16391


def test_b_the_clamps_and_a_tie_that_rounds_up():
    b, tr = P.cases(44100)["b"], dict(zip(P.cases(44100)["b"]["names"], P.truth(44100, "b")))
    t = tr["4Hz"]
    assert t["oi"].tolist() == [11024, 22049] and t["ot"].tolist() == [8192, 8192] and np.all(t["x"] > 8192.5)
    for k in ("21000Hz", "20000Hz", "14700Hz"):
        assert np.all(tr[k]["ot"] == 3) and tr[k]["oi"].size > 100
    assert np.all(tr["21000Hz"]["x"] < 2.5) and np.all(tr["20000Hz"]["x"] < 2.5)      # the clamp itself, not a rounding
    assert tr["21000Hz"]["C"].max() == 2                                              # three-sample pulses overlap
    assert np.all(tr["12600Hz"]["x"] == 3.5) and np.all(tr["12600Hz"]["ot"] == 4)
    tr = dict(zip(P.cases(96000)["b"]["names"], P.truth(96000, "b")))
    assert tr["4Hz"]["ot"].tolist() == [8192, 8192] and np.all(tr["4Hz"]["x"] > 8192.5)
    assert tr["4Hz"]["oi"][1] + 8192 <= tr["4Hz"]["n"]
    assert np.all(tr["47000Hz"]["ot"] == 3) and np.all(tr["47000Hz"]["x"] < 2.5) and tr["47000Hz"]["C"].max() == 2
    assert np.all(tr["12800Hz"]["x"] == 7.5) and np.all(tr["12800Hz"]["ot"] == 8)


@pytest.mark.parametrize("sr,note,x,T0,other,wrong", [
    (44100, "8Hz", 5512.5, 5512, "up", 5513), (22050, "4Hz", 5512.5, 5512, "up", 5513), (48000, "256Hz", 187.5, 188, "trunc", 187),
    (96000, "512Hz", 187.5, 188, "trunc", 187), (44100, "1800Hz", 24.5, 24, "up", 25)])
def test_c_exact_ties(sr, note, x, T0, other, wrong):
    b = P.cases(sr)["c"]
    k = b["names"].index(note)
    t = P.truth(sr, "c")[k]
    assert np.all(t["x"] == x) and np.all(t["ot"] == T0)          # exactly k + 0.5 in float64
    assert np.all(P.onsets(b["f0s"][k], sr, rounding=other)[2] == wrong)
    assert t["oi"].size >= 2 and t["oi"][1] + T0 + 8 == t["n"]    # two onsets and the whole second pulse


@pytest.mark.parametrize("f,sizes", [(11000, [510, 511, 512]), (11025, [512, 513, 513]), (13230, [614, 615, 615]), (21000, [975, 976, 976])])
def test_d_covering_lists_around_the_lds_list_s_size(f, sizes):
    b, tr = P.cases(44100)["d%d" % f], P.truth(44100, "d%d" % f)
    assert len(tr) == 1 and tr[0]["n"] == 3 * 2048 + 100                             # first (and alone) in its batch
    assert P.list_sizes([tr[0]["n"]], tr)[:3] == sizes
    assert P.MAXON == 512


def test_e_a_look_back_held_open():
    (t,) = P.truth(44100, "e")
    assert t["n"] == 17250
    assert t["oi"][0] == 7350 and t["ot"][0] == 7350 and t["oi"][1] == 7404 and np.all(t["ot"][1:] == 5)
    assert P.list_sizes([t["n"]], [t]) == [0, 0, 0, 162, 580, 998, 1416, 1834, 178]
    assert t["C"].max() == 3
    # the pulses themselves never reach back: without the running maximum the look-back would stop at once
    assert np.all(t["oi"][1:] + t["ot"][1:] <= t["oi"][1:] + 5)


def test_f_the_ragged_batch():
    b, tr = P.cases(44100)["f"], P.truth(44100, "f")
    lens = [t["n"] for t in tr]
    assert lens == [n + (P.F_HEAD if k % 2 else 0) for k, n in enumerate(P.F_LENGTHS)] and sum(lens) % 8 != 0
    for k, (n, f, t) in enumerate(zip(P.F_LENGTHS, b["f0s"], tr)):
        head = P.F_HEAD if k % 2 else 0
        assert not f[:head].any() and not t["C"][:head].any()
        if n >= 7:
            assert t["n"] - 3 <= t["oi"][-1] and t["oi"][-1] + t["ot"][-1] > t["n"]   # cut at the note's end
        else:
            assert t["oi"].size == 0
    assert P.list_sizes(lens, tr)[:3] == [None, None, None]                           # boundary tiles


def test_g_the_far_rows_under_other_models():
    for m, model in enumerate(P.LF_MODELS + (P.DEFAULT,)):
        b, tr = P.cases(44100)["g%d" % m], P.truth(44100, "g%d" % m)
        assert b["model"] == model and [int(t["ot"][0]) for t in tr] == [3, 2049, 8192]
    assert np.array_equal(P.truth(44100, "g3")[2]["pulse64"], P.truth(44100, "a")[17]["pulse64"])


# ---------------------------------------------------------------------------------------------
# planted faults
# ---------------------------------------------------------------------------------------------
CAUGHT_BY = {                                                 # fault: the batches that must see it
    "half_up": [(44100, "c"), (22050, "c")],
    "trunc": [(48000, "c"), (96000, "c"), (44100, "b")],
    "clamp_2048": [(44100, "a"), (44100, "b"), (96000, "b")],
    "clamp_2": [(44100, "b"), (96000, "b"), (44100, "d21000")],
    "row_offset": [(44100, "a"), (44100, "g1")],
    "row_short": [(44100, "a"), (44100, "g1")],
    "latest_three": [(44100, "e")],
    # (not d11025: its 513th onset starts on the tile's last sample, where it adds the shape's first value, an exact 0 — that
    # note reaches the per-sample path at its threshold, the two below show what a list cut short does)
    "first_512": [(44100, "d13230"), (44100, "d21000")],
    "own_end": [(44100, "e")],
    "no_cut": [(44100, "f")],
}


@functools.lru_cache(maxsize=None)
def _old_inputs():
    """The batches of tests/test_gpu_kernels.py's pulse tests, restated: (sr, model, f0s)"""
    res = []
    g = golden("pulse_train")
    res.append((44100, P.DEFAULT, [g["f0_" + k] for k in g["names"]]))
    res.append((96000, P.DEFAULT, [g["f0_sr96"]]))
    g = golden("pulse_train_lf")
    for model in g["models"]:
        res.append((int(g["sr"]), tuple(float(v) for v in model), [g["f0_" + str(k)] for k in g["names"]]))
    rng = np.random.default_rng(17)                           # test_pulse_train_many_random_notes_vs_oracle
    f0s = []
    for i in range(70):
        n = int(rng.integers(50, 9000))
        t = np.arange(n) / 44100
        base = rng.uniform(60, 900)
        f = base * 2 ** (rng.uniform(-0.5, 0.5) * np.sin(2 * np.pi * rng.uniform(1, 9) * t))
        f[rng.uniform(size=n) < 0.02] = 0
        if i % 7 == 0:
            f[:] = [440.0, 441.0, 220.5, 110.25, 882.0][i % 5]
        f0s.append(f.astype(F32))
    res.append((44100, P.DEFAULT, f0s))
    rng = np.random.default_rng(41)                           # test_pulse_onsets_parallel_scan_equals_sequential_walk
    f0s = []
    for i in range(44):
        n = int(rng.integers(20000, 70000)) if i < 30 else [1, 2, 511, 512, 513, 1023, 1024, 1025, 7, 64, 4096, 4097, 3000, 5000][i - 30]
        t = np.arange(n) / 44100
        f = rng.uniform(60, 900) * 2 ** (rng.uniform(-0.5, 0.5) * np.sin(2 * np.pi * rng.uniform(0.2, 9) * t))
        f[:int(0.08 * n)] = 0
        f[rng.uniform(size=n) < 0.01] = 0
        if i % 6 == 0:
            f[:] = [441.0, 220.5, 882.0, 110.25, 440.0][(i // 6) % 5]
        if i % 6 == 1:
            f[n // 3:n // 3 + 20] = -500.0
        if i % 6 == 2 and n > 100:
            f[int(rng.integers(50, n))] = 90000.0
        if i == 9:
            f[:] = 0
        f0s.append(f.astype(F32))
    res.append((44100, P.DEFAULT, [f for k, f in enumerate(f0s) if k % 3 == 0]))     # (the notes that test holds to the oracle)
    edge = []
    for i, n in enumerate([15, 16, 17, 31, 32, 33, 2047, 2048, 2049, 4095]):
        f = rng.uniform(4000, 9000) * 2 ** (0.3 * np.sin(2 * np.pi * rng.uniform(20, 200) * np.arange(n) / 44100))
        if i % 3 == 1:
            f[:] = 4410.0
        edge.append(f.astype(F32))
    res.append((44100, P.DEFAULT, edge))
    rng = np.random.default_rng(23)                           # test_pulse_train_negative_and_oversized_increments
    f0s = []
    for i in range(9):
        n = int(rng.integers(700, 4000))
        f = rng.uniform(150, 700) * np.ones(n)
        for _ in range(4):
            a = int(rng.integers(0, n - 60))
            f[a:a + int(rng.integers(1, 60))] = -rng.uniform(100, 3000)
        for _ in range(3):
            f[int(rng.integers(0, n))] = rng.uniform(50000, 140000)
        if i == 0:
            f[:] = -200.0
        f0s.append(f.astype(F32))
    res.append((44100, P.DEFAULT, f0s))
    return [(sr, model, f0s, np.concatenate([R.pulse_train(f, sr, *model) for f in f0s])) for sr, model, f0s in res]


def _old_rule_sees(fault):
    """the largest |faulty device - oracle| over the old inputs: the old tests assert < 4e-6 .. 5e-6 (the edge notes run in a
    batch of ten here; the old test also cuts them into smaller batches)"""
    return max(float(np.max(np.abs(P.device_model(f0s, sr, model, fault) - ref))) for sr, model, f0s, ref in _old_inputs())


def test_the_documented_device_passes_the_old_rule_on_the_old_inputs():
    assert _old_rule_sees(None) < 4e-6


@pytest.mark.parametrize("fault", P.FAULTS)
def test_planted_fault_falls_outside_the_bound(fault):
    seen = []
    for sr in P.RATES:
        for name, b in P.cases(sr).items():
            tr = P.truth(sr, name)
            v = P.judge(P.device_model(b["f0s"], sr, b["model"], fault), tr)
            if not v["ok"]:
                seen.append((sr, name, v["worst"]))
    old = _old_rule_sees(fault)
    print("FAULT %-13s outside the bound on %s; worst error / bound %.3g; the old rule on the old inputs: %s (largest error %.3g)"
          % (fault, ", ".join("%s@%d" % (n, sr) for sr, n, _ in seen), max([w for _, _, w in seen] or [0.0]),
             "seen" if old >= 5e-6 else "NOT seen", old))
    for want in CAUGHT_BY[fault]:
        assert want in [(sr, n) for sr, n, _ in seen], (fault, want, seen)
    assert max(w for _, _, w in seen) > 100.0                 # far outside, not marginally
