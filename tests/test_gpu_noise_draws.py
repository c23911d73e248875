"""GPU: the jitter (sh / sr) and growl (sj) draws made on the device (goofer_normal_fill, ``noise="device"``).

The stream is a definition (include/goofer_hip.h): tests/noise_ref.py restates it in numpy and the kernel's values are held
to it; the device's own output passes the statistics the restatement passes on the CPU (tests/test_noise_ref.py); a render
with device draws equals, bit for bit, the host-mode render that is handed the same draws, and stays within the parity
bound of the CPU oracle handed the same draws."""
import http.client
import threading

import numpy as np
import pytest

import noise_ref as NR
from conftest import rms_err
from goofer_amd import synthetic as syn

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ctx():
    from goofer_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _params(ids):
    from goofer_amd.device import default_params
    ids = np.asarray(ids, dtype=np.uint64)
    par = default_params(len(ids))
    par["seed"] = np.stack([ids & np.uint64(0xFFFFFFFF), ids >> np.uint64(32)], axis=1)
    return par


def _job(seed, flags, length_ms=300):
    from goofer_amd import sampler as S
    from goofer_amd.render import Source
    src = syn.make_source(seed, seconds=0.45)
    return (Source.from_pack(src["env_pack"], src["f0"], src["mask"], src["formants"], src["sr"], src["y_len"]),
            S.decode_request(*syn.request_args(syn.make_request(seed, flags, length_ms=length_ms))))


def _render(r, jobs, ids, seed):
    """the notes' mixes as device tensors, through prepare + run with explicit note ids"""
    prep = r.prepare(jobs, note_ids=ids)
    out = r.run(prep, seed=seed)
    r.ctx.check()
    off = prep["sample_off"]
    return [out["mix"][int(off[i]):int(off[i + 1])].clone() for i in range(len(jobs))]


def _boom(*a, **k):
    raise AssertionError("a host draw was made")


# ---- 1. the stream, value by value --------------------------------------------------------------------------------------
LENS = [1, 2, 3, 50001, 7, 0, 2, 1, 50000, 513, 1023, 3]                    # odd and even offsets, a note of no samples
IDS = [0, 1, (1 << 32) + 5, (3 << 40) + 9, 7, 8, 0xFFFFFFFFFFFFFFFF, 11, 12, (1 << 33) + 1, 14, 15]
ON = [1, 1, 1, 1, 0, 1, 1, 1, 0, 1, 1, 1]


@pytest.mark.parametrize("tag", range(5))
@pytest.mark.parametrize("masked", [False, True])
def test_stream_parity(ctx, tag, masked):
    seed = 0x1234ABCD5678EF01 + tag
    out = torch.full((sum(LENS),), -777.0, dtype=torch.float64, device=ctx.device)
    got = ctx.normal_fill(seed, _params(IDS), LENS, tag, note_on=ON if masked else None, out=out)
    assert got is out
    got = got.cpu().numpy()
    off = np.concatenate([[0], np.cumsum(LENS)])
    worst = 0.0
    for k, (n, nid) in enumerate(zip(LENS, IDS)):
        mine = got[off[k]:off[k + 1]]
        if masked and not ON[k]:
            assert (mine == -777.0).all(), k                 # a switched-off note keeps what was there
            continue
        ref = NR.normals(seed, nid, tag, n)
        if n:
            worst = max(worst, float(np.max(np.abs(mine - ref))))
    print("tag", tag, "worst |device - numpy|", worst)
    assert worst < 1e-13


def test_stream_parity_device_offsets_and_growl(ctx):
    """The renderer's calling form (device params and offsets) and the growl mode: 0.5 * 2^(scale z), 1e-13 relative."""
    seed, scale = 99, np.array([0.09, 0.0, 0.36, 0.01, 0.25, 1.0, 0.04, 0.09, 0.16, 0.09, 0.3, 0.5])
    o = ctx.device_offsets([1] * len(LENS), LENS, _params(IDS), hop=256)
    out = torch.full((sum(LENS),), -777.0, dtype=torch.float64, device=ctx.device)
    ctx.normal_fill(seed, o["d_par"], o["d_s"], 4, note_on=ON, growl_scale=scale, out=out)
    plain = ctx.normal_fill(seed, _params(IDS), LENS, 4).cpu().numpy()
    got = out.cpu().numpy()
    off = np.concatenate([[0], np.cumsum(LENS)])
    worst = 0.0
    for k, (n, nid) in enumerate(zip(LENS, IDS)):
        mine = got[off[k]:off[k + 1]]
        if not ON[k]:
            assert (mine == -777.0).all()
            continue
        ref = 0.5 * 2.0 ** (scale[k] * NR.normals(seed, nid, 4, n))
        assert np.max(np.abs(plain[off[k]:off[k + 1]] - NR.normals(seed, nid, 4, n)), initial=0.0) < 1e-13
        if n:
            worst = max(worst, float(np.max(np.abs(mine - ref) / ref)))
    print("growl worst relative", worst)
    assert worst < 1e-13
    ref = NR.growl(seed, IDS[0], LENS[0], 0.3)
    assert abs(float(got[0]) - ref[0]) / ref[0] < 1e-13 and scale[0] == 0.3 ** 2


# ---- 2. statistics of the device's own output ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(NR.STAT_KEYS)))
def test_device_output_statistics(ctx, case):
    seed, note = NR.STAT_KEYS[case]
    tag, n = case % 5, NR.STAT_N
    draw = lambda nid, t: ctx.normal_fill(seed, _params([nid]), [n], t).cpu().numpy()
    z = draw(note, tag)
    NR.assert_normal(z, f"device key {case} tag {tag}")
    c = NR.correlation(z, draw(note, (tag + 1) % 5))
    print("cross-stream", round(c, 3))
    assert c < NR.SE_MAX
    c = NR.correlation(z, draw(note + 1, tag))               # two notes that differ only in id
    print("cross-note", round(c, 3))
    assert c < NR.SE_MAX


# ---- 3. a note's draws are its own --------------------------------------------------------------------------------------
FLAGS = ["sh50sr50", "sj30", "sh50sr50sj30", "t0g0"]


def _mixed_jobs(k=0):
    return [_job(300 + 10 * k + j, FLAGS[j], length_ms=220 + 45 * j + 10 * k) for j in range(4)]


def test_notes_render_alike_alone_in_any_batch_and_pipelined(ctx):
    from goofer_amd.render import PipelinedRenderer, Renderer
    r = Renderer(ctx, noise="device")
    jobs, ids, seed = _mixed_jobs(), [(1 << 32) + 40, 41, 42, 43], 2026
    batch = _render(r, jobs, ids, seed)
    for i in range(4):
        (alone,) = _render(r, [jobs[i]], [ids[i]], seed)
        assert torch.equal(alone, batch[i]), i
    back = _render(r, jobs[::-1], ids[::-1], seed)
    for i in range(4):
        assert torch.equal(back[3 - i], batch[i]), i
    other = _render(r, jobs, ids, seed + 1)
    for i in range(3):                                        # another seed: other draws (and other phases)
        assert not torch.equal(other[i], batch[i])
    moved = _render(r, jobs, [i + 1000 for i in ids], seed)
    assert not torch.equal(moved[0], batch[0])
    # the same four caller batches through the pipeline, one device batch each and all four as one
    batches = [_mixed_jobs(k) for k in range(4)]
    note_ids = lambda k, n: [5000 + 16 * k + j for j in range(n)]
    want = [_render(r, batches[k], note_ids(k, 4), seed) for k in range(4)]
    for coalesce in (1, 4):
        pr = PipelinedRenderer(depth=2, workers=2, coalesce=coalesce, noise="device")
        try:
            got = pr.render_all([([j[0] for j in b], [j[1] for j in b]) for b in batches], seed=seed, note_ids=note_ids)
        finally:
            pr.close()
        for k in range(4):
            for j in range(4):
                assert torch.equal(torch.from_numpy(got[k][j]), want[k][j].cpu()), (coalesce, k, j)


# ---- 4. no host draws ---------------------------------------------------------------------------------------------------
def test_device_noise_makes_no_host_draw(ctx, monkeypatch):
    from goofer_amd.render import Renderer
    jobs = [_job(400, "sh50sr50sj30"), _job(401, "sh50sr50sj30", 260), _job(402, "t0g0")]
    monkeypatch.setattr(np.random, "randn", _boom)
    monkeypatch.setattr(np.random, "default_rng", _boom)
    outs = Renderer(ctx, noise="device").render(jobs, seed=5)
    assert all(np.isfinite(o).all() and np.abs(o).max() > 1e-3 for o in outs)
    with pytest.raises(AssertionError, match="a host draw was made"):     # the replacement bites
        Renderer(ctx, noise="host").render(jobs, seed=5)
    with pytest.raises(AssertionError, match="a host draw was made"):
        Renderer(ctx).render(jobs[:1], seed=5)                            # (host is the default)


# ---- 5. the same kernels downstream -------------------------------------------------------------------------------------
def test_host_mode_handed_the_device_draws_renders_the_same_bits(ctx, monkeypatch):
    from goofer_amd.render import Renderer
    flags = ["sh50sr50", "sr40", "sh30sr60", "sh70sr20"]
    jobs = [_job(500 + j, flags[j], length_ms=230 + 50 * j) for j in range(4)]
    seed, phi = 77, [9000, 9001, 9002, 9003]
    r, rd = Renderer(ctx), Renderer(ctx, noise="device")
    dev = [torch.from_numpy(o) for o in rd.render(jobs, seed=seed, phi_seeds=phi)]
    lens = rd.prepare(jobs)["lens"]
    off = np.concatenate([[0], np.cumsum(lens)])
    z = [ctx.normal_fill(seed, _params(range(4)), lens, tag).cpu().numpy() for tag in (0, 1, 2)]
    queue = []                                               # prepare's call order: per note f0 (sh), harmonic, breath (sr)
    for j, f in enumerate(flags):
        queue += [z[t][off[j]:off[j + 1]] for t in ((0, 1, 2) if "sh" in f else (1, 2))]

    def randn(n):
        d = queue.pop(0)
        assert d.size == n
        return d.copy()
    monkeypatch.setattr(np.random, "randn", randn)
    host = [torch.from_numpy(o) for o in r.render(jobs, seed=seed, phi_seeds=phi)]
    assert not queue
    for j in range(4):
        assert torch.equal(host[j], dev[j]), j


# ---- 6. against the oracle directly -------------------------------------------------------------------------------------
class _Rng:
    """default_rng(seed) as the oracle uses it: the phases' uniform is the real generator's, normal() hands out the growl draws"""

    def __init__(self, real, z4):
        self.uniform, self.z4 = real.uniform, z4

    def normal(self, loc=0.0, scale=1.0, size=None):
        assert loc == 0.0 and size == self.z4.size
        return scale * self.z4


@pytest.mark.parametrize("config,ids,flags", [(3, [0, 1, 2, 3, 257, 512, 777, 1023], "sh50sr50"), (5, [0, 1, 512, 1023], "sh50sr50"),
                                              (3, [4, 5, 640, 900], "sj30")])
def test_device_draws_vs_oracle(config, ids, flags):
    from goofer_amd.device import Context
    from goofer_amd.render import Renderer, Source
    from goofer_amd import sampler as S
    from oracle import sampler_ref as SR
    geo = syn.config_geometry(config)
    c = Context(0)
    real_randn, real_rng = np.random.randn, np.random.default_rng
    try:
        r = Renderer(c, hop=geo["hop"], noise="device")
        jobs, feats, reqs, seeds = [], [], [], []
        for i in ids:
            src, req, phi_seed = syn.config_note(config, i)
            req = dict(req, flags=req["flags"] + flags)
            jobs.append((Source.from_pack(src["env_pack"], src["f0"], src["mask"], src["formants"], src["sr"], src["y_len"]),
                         S.decode_request(*syn.request_args(req))))
            feats.append((src["env_pack"], src["f0"].copy(), src["mask"].copy(), {k: v.copy() for k, v in src["formants"].items()},
                          src["sr"], src["y_len"]))
            reqs.append(req)
            seeds.append(phi_seed)
        seed = 31337
        outs = r.render(jobs, seed=seed, phi_seeds=seeds)
        lens = r.prepare(jobs)["lens"]
        off = np.concatenate([[0], np.cumsum(lens)])
        z = [c.normal_fill(seed, _params(range(len(ids))), lens, tag).cpu().numpy() for tag in (0, 1, 2, 4)]
        for j, i in enumerate(ids):
            queue = [z[t][off[j]:off[j + 1]] for t in (0, 1, 2)]      # the oracle's order: f0, harmonic, breath

            def randn(n):
                d = queue.pop(0)
                assert d.size == n
                return d.copy()
            np.random.randn = randn
            np.random.default_rng = lambda sd=None, j=j: _Rng(real_rng(sd), z[3][off[j]:off[j + 1]])
            try:
                ref = SR.render(feats[j], SR.decode_request(*syn.request_args(reqs[j])), seed=seeds[j], n_fft=geo["n_fft"], hop=geo["hop"])
            finally:
                np.random.randn, np.random.default_rng = real_randn, real_rng
            assert len(queue) == (0 if "sh" in flags else 3)          # the oracle drew what the flags say
            assert outs[j].shape == ref.shape
            e = rms_err(outs[j], ref) / max(1.0, float(np.max(np.abs(ref))))
            print("config", config, "note", i, flags, "rms_err / max(1, peak)", e)
            assert e < 2e-5, (config, i, e)
    finally:
        np.random.randn, np.random.default_rng = real_randn, real_rng
        c.close()


# ---- 7. ABI refusals ----------------------------------------------------------------------------------------------------
def test_abi_refusals(ctx):
    from goofer_amd.device import GooferError, _ptr
    sentinel = torch.full((8,), -5.0, dtype=torch.float64, device=ctx.device)
    o = ctx.device_offsets([1, 1], [3, 5], _params([1, 2]), hop=256)
    call = lambda n, total, tag, out: ctx._check(ctx.lib.goofer_normal_fill(ctx.h, 1, _ptr(o["d_par"]), _ptr(o["d_s"]), n, total, tag, None,
                                                                            None, out, ctx._stream()))
    with pytest.raises(GooferError, match="null pointer"):
        call(2, 8, 0, None)
    with pytest.raises(GooferError, match="tag 5"):
        call(2, 8, 5, _ptr(sentinel))
    with pytest.raises(GooferError, match="tag 5"):
        ctx.normal_fill(1, _params([1, 2]), [3, 5], 5, out=sentinel)
    with pytest.raises(GooferError, match="negative count"):
        call(-1, 8, 0, _ptr(sentinel))
    torch.cuda.synchronize()
    assert (sentinel == -5.0).all()                          # nothing was launched
    call(2, 8, 0, _ptr(sentinel))
    assert (sentinel != -5.0).all()


# ---- 8. the front end ---------------------------------------------------------------------------------------------------
def test_environment_reaches_the_front_end(tmp_path, monkeypatch):
    from goofer_amd import cli, core
    from goofer_amd.render import GooferResampler, Renderer
    bodies = []
    for i in range(2):
        src = syn.make_source(600 + i, seconds=0.4)
        wav = tmp_path / f"s{i}.wav"
        core.save_features(wav.with_name(f"s{i}_features.goofy"), src["env_pack"], src["f0"], src["mask"], src["formants"], src["sr"], src["y_len"])
        bodies.append([str(wav), str(tmp_path / f"o{i}.wav")] + syn.request_args(syn.make_request(600 + i, "sh50", length_ms=250)))
    monkeypatch.setenv("GOOFER_NOISE", "bogus")
    with pytest.raises(ValueError, match="bogus"):
        cli.BatchCollector()
    with pytest.raises(ValueError, match="bogus"):
        GooferResampler(*bodies[0])
    assert cli.main(bodies[0]) == 1 and not (tmp_path / "o0.wav").exists()
    with pytest.raises(ValueError, match="bogus"):
        Renderer(noise=None)
    monkeypatch.setenv("GOOFER_NOISE", "device")
    monkeypatch.setattr(np.random, "randn", _boom)
    monkeypatch.setattr(np.random, "default_rng", _boom)
    assert cli.main(bodies[0]) == 0 and (tmp_path / "o0.wav").stat().st_size > 44     # the 13-argument call
    collector = cli.BatchCollector(window_s=0.01)
    assert collector.noise == "device"
    httpd, _ = cli.serve(0, collector, host="127.0.0.1")
    th = threading.Thread(target=httpd.serve_forever, daemon=True)
    th.start()
    try:
        conn = http.client.HTTPConnection("127.0.0.1", httpd.server_address[1], timeout=120)
        conn.request("POST", "/", body=" ".join(bodies[1]).encode("utf-8"))
        resp = conn.getresponse()
        assert (resp.status, resp.read().decode()) == (200, "")
        conn.close()
        assert all(r.noise == "device" for r, _ in collector._lane_list())
        assert (tmp_path / "o1.wav").stat().st_size > 44
        monkeypatch.setenv("GOOFER_NOISE", "host")            # ... and the host source does draw on this path
        with pytest.raises(AssertionError, match="a host draw was made"):
            GooferResampler(*bodies[0])
    finally:
        httpd.shutdown()
        collector.close()
