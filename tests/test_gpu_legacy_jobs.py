"""GPU: goofer_legacy_normal_jobs (k_legacy_normal_jobs, noise.hip) against the restatement of its job rule
(tests/legacy_jobs_ref.py over tests/mt_ref.py, which reproduce numpy's ``np.random.seed(s); np.random.randn(n)`` bit for bit on the
host), and against goofer_legacy_normal_fill on the same inputs.

The bound is the one tests/test_gpu_legacy_fill.py derives for this arithmetic: everything but ``log`` is exact and the acceptance
of an attempt does not depend on ``log``, so attempts are compared exactly and values within relative 1e-14 (a few ulps of the
device's against the host's ``log``, carried through one division, one square root and one product).  The float32-rounded
values are held to the same bound: rounding moves one only where its float64 value lies within those ulps of a float32 rounding
boundary (about one sample in 10^8), and the seeds here are fixed."""
import ctypes as C

import numpy as np
import pytest

import legacy_jobs_ref as J

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD = 64
BIG = 20011                                                    # many blocks


@pytest.fixture(scope="module")
def ctx():
    from goofer_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _table():
    """~24 ragged jobs as (seed, n, [arena name or None per destination], f32): every size with 1-4 destinations, null
    destinations in front, in the middle and behind, the float32 switch, n = 0 and no destination"""
    rows = [
        (0, 1, "x", 0), (1, 1, "xyxy", 0), (4027, 2, "xy", 0), (2 ** 32 - 1, 2, "yxy", 1),
        (5, 61, "xyxy", 0),                                    # 244 normals: one short of the average block
        (6, 61, "x-y", 0), (7, 61, "y", 1), (8, 123, "xy", 0), (9, 123, "-x", 0), (10, 123, "xyx", 1), (11, 123, "yxyx", 0),
        (1337, 1501, "x", 1), (1338, 1501, "y", 1), (1339, 1501, "x", 1),            # the roughness jobs of three partials
        (12, 1501, "xyxy", 0), (13, 1501, "xy-", 0), (2 ** 32 - 1, 1501, "y-xy", 0), (0, 1501, "yx", 0), (14, 1501, "---", 0),
        (15, 0, "xy", 0), (16, 61, "", 0), (17, 0, "", 1),     # nothing drawn
        (4027, BIG, "xy", 0), (18, 2, "x", 1),
    ]
    return [(s, n, [None if ch == "-" else ch for ch in d], bool(f)) for s, n, d, f in rows]


@pytest.fixture(scope="module")
def plan():
    """the table laid out over two NaN arenas with guard bands in front of, between and behind the destinations, and the
    restatement's result for it"""
    size = {"x": GUARD, "y": GUARD}
    table = []
    for seed, n, names, f32 in _table():
        dsts = []
        for name in names:
            if name is None:
                dsts.append(None)
                continue
            dsts.append((name, size[name]))
            size[name] += n + GUARD
        table.append((seed, n, dsts, f32))
    ref = {k: np.full(v, np.nan) for k, v in size.items()}
    attempts = J.run(table, ref)
    for a in ref.values():
        a.setflags(write=False)
    return {"table": table, "size": size, "ref": ref, "attempts": attempts}


def _arenas(ctx, size):
    return {k: torch.full((v,), float("nan"), dtype=torch.float64, device=ctx.device) for k, v in size.items()}


def _device_table(table, arenas):
    return [(s, n, [None if d is None else (arenas[d[0]], d[1]) for d in dsts], f32) for s, n, dsts, f32 in table]


@pytest.mark.parametrize("wave", [0, 1])
def test_ragged_job_table_against_the_restatement(ctx, plan, wave):
    arenas = _arenas(ctx, plan["size"])
    ctx.set_option("legacy_wave", wave)
    try:
        att = ctx.legacy_normal_jobs(_device_table(plan["table"], arenas), attempts=True)
        ctx.check()
    finally:
        ctx.set_option("legacy_wave", 0)
    assert np.array_equal(att.cpu().numpy(), plan["attempts"])               # the acceptances: exactly the restatement's
    for name, ref in plan["ref"].items():
        z = arenas[name].cpu().numpy()
        written = ~np.isnan(ref)
        assert np.array_equal(~np.isnan(z), written), name                   # guard bands and everything unaddressed: intact
        rel = np.abs(z[written] - ref[written]) / np.abs(ref[written])
        print(f"legacy_wave={wave} arena {name}: {int(written.sum())} normals, worst relative difference {rel.max():.3e}, "
              f"bit-equal {100.0 * float((z[written] == ref[written]).mean()):.3f} %")
    f32_values = 0
    for seed, n, dsts, f32 in plan["table"]:
        for d in dsts:
            if d is None or n == 0:
                continue
            z = arenas[d[0]][d[1]:d[1] + n].cpu().numpy()
            r = plan["ref"][d[0]][d[1]:d[1] + n]
            if f32:
                assert np.array_equal(z, z.astype(np.float32).astype(np.float64))          # exactly float32-representable
                f32_values += n
            assert float((np.abs(z - r) / np.abs(r)).max()) <= 1e-14
    assert f32_values > 4000
    m = np.array([n * len(d) for _, n, d, _ in plan["table"]])
    assert ((-(-plan["attempts"] // 156)) <= 2 * -(-m // 245) + 4).all()     # no job came near its block bound


def test_a_job_draws_the_same_bits_alone_and_in_the_table(ctx, plan):
    arenas = _arenas(ctx, plan["size"])
    att = ctx.legacy_normal_jobs(_device_table(plan["table"], arenas), attempts=True)
    for j in (1, 9, 12, 16, 3):                                # four destinations, a null one in front, odd n, null in the middle, float32
        seed, n, dsts, f32 = plan["table"][j]
        alone = [None if d is None else torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float64, device=ctx.device) for d in dsts]
        a1 = ctx.legacy_normal_jobs([(seed, n, [None if t is None else (t, GUARD) for t in alone], f32)], attempts=True)
        ctx.check()
        assert int(a1[0]) == int(att[j])
        for d, t in zip(dsts, alone):
            if d is not None:
                assert torch.equal(t[GUARD:GUARD + n], arenas[d[0]][d[1]:d[1] + n]), j
                assert bool(torch.isnan(t[:GUARD]).all()) and bool(torch.isnan(t[GUARD + n:]).all())


def test_the_old_entry_point_is_the_job_table_of_a_notes_enabled_streams(ctx):
    """goofer_legacy_normal_fill and a job table of three destinations (and the other on-patterns' one and two): the same bits
    and the same attempts"""
    lens = [1, 2, 61, 123, 1501, 123, 61, 1501, 0, 311]
    on = [(1, 1, 1)] * 5 + [(1, 0, 1), (0, 1, 1), (1, 0, 0), (1, 1, 1), (0, 0, 0)]
    seeds = [0, 1, 4027, 2 ** 32 - 1, 77, 78, 79, 80, 81, 82]
    off = np.concatenate([[0], np.cumsum(lens)])
    total = int(off[-1])
    for wave in (0, 1):
        ctx.set_option("legacy_wave", wave)
        try:
            old = tuple(torch.full((total,), float("nan"), dtype=torch.float64, device=ctx.device) for _ in range(3))
            _, a_old = ctx.legacy_normal_fill(seeds, lens, on, out=old, attempts=True)
            new = tuple(torch.full((total,), float("nan"), dtype=torch.float64, device=ctx.device) for _ in range(3))
            table = [(s, n, [(new[k], int(off[i])) for k in range(3) if o[k]], False) for i, (s, n, o) in enumerate(zip(seeds, lens, on))]
            a_new = ctx.legacy_normal_jobs(table, attempts=True)
            ctx.check()
        finally:
            ctx.set_option("legacy_wave", 0)
        assert torch.equal(a_old, a_new)
        for a, b in zip(old, new):
            assert torch.equal(torch.isnan(a), torch.isnan(b))
            assert torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0))
        assert int(torch.isnan(old[0]).sum()) == 61 + 311 and int(a_old[8]) == 0


def test_bad_arguments_are_refused_before_a_launch(ctx, monkeypatch):
    from goofer_amd.device import GooferError
    good = torch.full((32,), float("nan"), dtype=torch.float64, device=ctx.device)
    launched = []
    real = ctx.lib.goofer_legacy_normal_jobs
    monkeypatch.setattr(ctx.lib, "goofer_legacy_normal_jobs", lambda *a: launched.append(a) or real(*a))
    bad_tables = [
        [(1, 30, [(good, 3)], False)],                         # past the end
        [(1, 4, [(good, -1)], False)],
        [(1, -4, [(good, 0)], False)],
        [(1, 4, [(good, 0)] * 5, False)],                      # five destinations
        [(1, 4, [(good.float(), 0)], False)],
        [(1, 4, [(good.cpu(), 0)], False)],
        [(1, 4, [(good[::2], 0)], False)],
        [(1, 4, [(good, 0)], False), (2 ** 32, 4, [(good, 8)], False)],      # one bad job refuses the whole table
        [(-1, 4, [(good, 0)], False)], [(None, 4, [(good, 0)], False)], [(1.5, 4, [(good, 0)], False)], [(True, 4, [(good, 0)], False)],
        [(1, 4)],
    ]
    for t in bad_tables:
        with pytest.raises(ValueError):
            ctx.legacy_normal_jobs(t)
    assert launched == []
    monkeypatch.undo()
    tab = torch.zeros(88, dtype=torch.uint8, device=ctx.device)              # one job that draws nothing
    att = torch.full((2,), -1, dtype=torch.int64, device=ctx.device)
    call = lambda *a: ctx.lib.goofer_legacy_normal_jobs(ctx.h, *a, ctx._stream())   # noqa: E731
    for args in ((None, 1, C.c_void_p(att.data_ptr())), (C.c_void_p(tab.data_ptr()), -1, None),
                 (C.c_void_p(tab.data_ptr() + 4), 0, None), (C.c_void_p(tab.data_ptr()), 1, C.c_void_p(att.data_ptr() + 4))):
        with pytest.raises(GooferError):
            ctx._check(call(*args))
    ctx.check()
    assert bool(torch.isnan(good).all()) and bool((att == -1).all())         # nothing ran
    assert ctx.legacy_normal_jobs([]) is None and ctx.legacy_normal_jobs([], attempts=True).numel() == 0
