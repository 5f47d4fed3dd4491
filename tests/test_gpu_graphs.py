"""The forms bench.py times, on the MI355X (pytest -m gpu): every engine program replayed as a hipGraph, the denoise step with its
two lanes (ControlNet / UNet encoder + middle block) as two parallel graph branches, and two engine slots in flight on two
streams.  Every other CLDM / VAE test replays the launch list eagerly, in list order, on one stream, in slot 0.

Eager replay is the reference here and is already anchored: tests/test_gpu_e2e.py and tests/test_gpu_mixed.py hold it against
the reference's goldens, and it is deterministic (test_full_size_batch_invariance_and_determinism).  This file proves that the
captured forms are the SAME function: every assertion is torch.equal on fp32 outputs, bit for bit.  A difference is a finding —
a buffer both lanes touch, an argument frozen at capture, a buffer two slots share — never noise.  The host-side rules that go
with it (which memory the lanes and the slots may share) are in tests/test_lanes_cpu.py.

Each graph is replayed three times at the most (inputs A, B, A: the graph reads its inputs through the engine's static buffers,
nothing by-value was frozen), except in the four-step sampler flow of the last test, where each of the four replays of the
step graph has another input."""
import pytest
import torch

pytestmark = pytest.mark.gpu

USED = [50, 100, 150, 200]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def models():
    """One model per (configuration, dtype, precision) for the whole file: the weights are packed once."""
    from edtr_amd import synth
    from edtr_amd.testing import build_synthetic_cldm
    made = {}

    def get(config, dtype, precision):
        key = (config, dtype, precision)
        if key not in made:
            made[key] = build_synthetic_cldm(synth.CONFIGS[config](), _dev(), dtype, precision=precision)
        return made[key]

    yield get
    for m in made.values():
        m.release_engines()


def _step_inputs(tag, B, h, w, ctx_dim, dev):
    """Inputs A and B of one denoise step: (x, t, c_txt, c_img) each, in CldmEngine.step's order."""
    from edtr_amd import synth
    out = []
    for name, t in (("A", 200), ("B", 50)):
        x = synth.synth_normal(f"graphs:{tag}:{name}:x", (B, 4, h, w)).to(dev)
        c_img = synth.synth_normal(f"graphs:{tag}:{name}:c_img", (B, 4, h, w)).to(dev)
        c_txt = synth.synth_input(f"graphs:{tag}:{name}:c_txt", (B, 77, ctx_dim), -1.0, 1.0).to(dev)
        out.append((x, torch.full((B,), t, dtype=torch.int64, device=dev), c_txt, c_img))
    return out


def _eager_step(eng, inp):
    assert eng.step_prog.graph is None
    out = eng.step(*inp).clone()
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and out.dtype == torch.float32
    return out


@pytest.mark.parametrize("dtype,precision,B,h,w", [(torch.float16, "fast", 2, 16, 16), (torch.bfloat16, "fast", 2, 16, 16),
                                                    (torch.bfloat16, "fast", 1, 24, 16), (None, "mixed", 2, 16, 16)])
def test_step_graph_equals_eager(models, dtype, precision, B, h, w):
    """The serial capture (both lanes on one stream) separates "capture itself changes something" from "the lanes race"."""
    dev = _dev()
    cldm = models("tiny", dtype, precision)
    A, Bi = _step_inputs("step", B, h, w, 64, dev)
    eng = cldm.cldm_engine(B, h, w)
    eA, eB = _eager_step(eng, A), _eager_step(eng, Bi)
    assert not torch.equal(eA, eB)
    for parallel in (False, True):
        eng.step_prog.capture(parallel_lanes=parallel)
        try:
            assert eng.step_prog.graph is not None
            got = [eng.step(*inp).clone() for inp in (A, Bi, A)]
            torch.cuda.synchronize()
        finally:
            torch.cuda.synchronize()
            eng.step_prog.release_graph()
        for g, want, name in zip(got, (eA, eB, eA), "ABA"):
            assert torch.equal(g, want), f"parallel_lanes={parallel}, input {name}: {int((g != want).sum())} of {g.numel()} elements differ"
    assert torch.equal(_eager_step(eng, Bi), eB)                   # and the engine is back to its launch list


@pytest.mark.parametrize("B,h,w", [(2, 32, 32), (8, 64, 64)])
def test_step_graph_equals_eager_at_sd21_widths(models, B, h, w):
    """SD-2.1 widths.  (2, 32, 32): the smallest latents that reach all four UNet levels — split-K products with their reducer and
    the concat-slot GroupNorm are in the program.  edtr_ffn and edtr_lin320 are not: they take 16384 / 32768 rows and more
    (ops.ffn_ok, ops.lin320_ok), so the second case is the benchmark's own shape, where both are.  One eager run and one replay
    of the parallel capture each, on input A only."""
    from edtr_amd import lib
    dev = _dev()
    cldm = models("sd21", torch.bfloat16, "fast")
    A, _ = _step_inputs("sd21", B, h, w, 1024, dev)
    eng = cldm.cldm_engine(B, h, w)
    recs = eng.step_prog.recs
    assert any(" sk" in r.tag for r in recs) and any(r.name == "gn.finalize" for r in recs)
    big = B * h * w >= 32768
    assert any(r.fn is lib.load().edtr_ffn for r in recs) == big and any(r.fn is lib.load().edtr_lin320 for r in recs) == big
    eA = _eager_step(eng, A)
    eng.step_prog.capture(parallel_lanes=True)
    try:
        gA = eng.step(*A).clone()
        torch.cuda.synchronize()
    finally:
        torch.cuda.synchronize()
        eng.step_prog.release_graph()
    assert torch.equal(gA, eA), f"{int((gA != eA).sum())} of {gA.numel()} elements differ"


def test_vae_graphs_equal_eager(models):
    """Encoder, decoder and the two tiled forms through the public methods.  The tiled forms skip their NaN probe only while
    they are being captured: a captured replay still runs it."""
    from edtr_amd import synth
    from edtr_amd.testing import capture_engines, release_graphs
    dev = _dev()
    cldm = models("tiny", torch.bfloat16, "fast")
    release_graphs(cldm)

    def img(name, shape):
        return synth.synth_input(f"graphs:vae:{name}", shape, -1.0, 1.0).to(dev)

    def lat(name, shape):
        return synth.synth_normal(f"graphs:vae:{name}", shape).to(dev)

    forms = {
        "encode": (lambda x: cldm.vae_encode(x, sample=False), [img(f"enc{k}", (2, 3, 128, 128)) for k in "AB"]),
        "decode": (lambda z: cldm.vae_decode(z), [lat(f"dec{k}", (2, 4, 16, 16)) for k in "AB"]),
        "decode.tiled": (lambda z: cldm.vae_decode(z, tiled=True, tile_size=16), [lat(f"tdec{k}", (1, 4, 40, 40)) for k in "AB"]),
        "encode.tiled": (lambda x: cldm.vae_encode(x, sample=False, tiled=True, tile_size=128), [img(f"tenc{k}", (1, 3, 320, 320)) for k in "AB"]),
    }
    eager = {k: [f(a), f(b)] for k, (f, (a, b)) in forms.items()}            # (builds and caches the four engines)
    torch.cuda.synchronize()
    engines = list(cldm._vae_engines.values())
    assert sum(e.nan_probe is not None for e in engines) == 2 and all(e.prog.graph is None for e in engines)
    assert all(torch.isfinite(t).all() and not torch.equal(a, b) for a, b in eager.values() for t in (a, b))
    capture_engines(cldm)
    try:
        assert all(e.prog.graph is not None for e in engines)
        got = {k: [f(a), f(b), f(a)] for k, (f, (a, b)) in forms.items()}
        torch.cuda.synchronize()
    finally:
        release_graphs(cldm)
    assert all(e.prog.graph is None for e in engines)
    for k, (gA, gB, gA2) in got.items():
        eA, eB = eager[k]
        assert torch.equal(gA, eA) and torch.equal(gB, eB) and torch.equal(gA2, eA), k


def test_two_slots_in_flight_equal_one_at_a_time(models):
    """bench.py's run_steps at --inflight 2: slot 0 and slot 1, both captured with parallel lanes, replayed back to back on two
    streams with no synchronisation between them."""
    from edtr_amd.testing import release_graphs
    dev = _dev()
    cldm = models("tiny", torch.bfloat16, "fast")
    release_graphs(cldm)
    B, h, w = 2, 16, 16
    A, Bi = _step_inputs("slots", B, h, w, 64, dev)
    try:
        cldm.engine_slot = 0
        e0 = cldm.cldm_engine(B, h, w)
        eA, eB = _eager_step(e0, A), _eager_step(e0, Bi)
        cldm.engine_slot = 1
        e1 = cldm.cldm_engine(B, h, w)
    finally:
        cldm.engine_slot = 0
    assert e1 is not e0 and not torch.equal(eA, eB)
    assert torch.equal(_eager_step(e1, A), eA)                      # (the warm-up pass of slot 1, as in the benchmark)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for e in (e0, e1):
        e.step_prog.capture(parallel_lanes=True)
    try:
        for st in streams:
            st.wait_stream(torch.cuda.current_stream())
        got = []
        for first, second in ((A, Bi), (Bi, A)):
            with torch.cuda.stream(streams[0]):
                got.append(e0.step(*first).clone())
            with torch.cuda.stream(streams[1]):
                got.append(e1.step(*second).clone())
        for st in streams:
            torch.cuda.current_stream().wait_stream(st)
        torch.cuda.synchronize()
    finally:
        release_graphs(cldm)
    for g, want, name in zip(got, (eA, eB, eB, eA), ("slot 0: A", "slot 1: B", "slot 0: B", "slot 1: A")):
        assert torch.equal(g, want), f"{name}: {int((g != want).sum())} of {g.numel()} elements differ"


def test_tiny_flow_captured_equals_eager(models):
    """The flow of test_gpu_e2e._run twice on one model object — vae_encode, q_sample, four sampler steps with injected noise,
    vae_decode — once eagerly (that pass builds and caches the engines) and once with the engines' programs in graphs, as in the
    benchmark: only they are captured, the sampler's own launches stay eager."""
    from edtr_amd import synth
    from edtr_amd.diffusion import Diffusion
    from edtr_amd.sampler import SpacedSampler
    from edtr_amd.testing import capture_engines, injected_noise, release_graphs
    dev = _dev()
    cldm = models("tiny", torch.bfloat16, "fast")
    release_graphs(cldm)
    B, H, W = 2, 128, 128
    diffusion = Diffusion(linear_start=0.00085, linear_end=0.0120, timesteps=1000).to(dev)
    sampler = SpacedSampler(diffusion.betas)
    pre_res = synth.synth_input("graphs:flow:pre_res", (B, 3, H, W), 0.0, 1.0).to(dev)
    c_txt = synth.synth_input("graphs:flow:c_txt", (B, 77, 64), -1.0, 1.0).to(dev)
    noises = [synth.synth_normal(f"graphs:flow:noise{i}", (B, 4, H // 8, W // 8)).to(dev) for i in range(5)]

    def flow():
        z_pre = cldm.vae_encode(pre_res * 2 - 1, sample=False)
        x_T = diffusion.q_sample(z_pre, torch.full((B,), 200, dtype=torch.int64, device=dev), noises[0])
        eps_log = []

        def logging_forward(x, t, cond, woSD=False):
            e = type(cldm).forward(cldm, x, t, cond)
            eps_log.append(e.clone())
            return e

        cldm.forward = logging_forward
        try:
            with injected_noise(noises[1:]):
                z = sampler.manual_sample_with_timesteps(
                    model=cldm, device=dev, x_T=x_T, steps=4, used_timesteps=USED, batch_size=B,
                    cond={"c_txt": c_txt, "c_img": z_pre}, uncond=None, cfg_scale=1.0, progress=False)
        finally:
            del cldm.forward
        img = cldm.vae_decode(z)
        torch.cuda.synchronize()
        assert len(eps_log) == 4
        return dict(z_pre=z_pre, z=z, img=img, **{f"eps{i}": e for i, e in enumerate(eps_log)})

    eager = flow()
    programs = [e.step_prog for e in cldm._cldm_engines.values()] + [e.prog for e in cldm._vae_engines.values()]
    assert len(programs) >= 3 and all(p.graph is None for p in programs)
    capture_engines(cldm)
    try:
        assert all(p.graph is not None for p in programs)
        captured = flow()
    finally:
        release_graphs(cldm)
    assert all(torch.isfinite(v).all() for v in eager.values())
    for k in ("z_pre", "eps0", "eps1", "eps2", "eps3", "z", "img"):
        assert torch.equal(captured[k], eager[k]), f"{k}: {int((captured[k] != eager[k]).sum())} of {eager[k].numel()} elements differ"
