"""Seeded per-image noise on the device (csrc/rng.hip, include/edtr_hip.h "Reproducible noise"): the stand-alone fill against the
numpy restatement of edtr_amd/rng.py, the fused kernels against "fill, then the tensor-noise kernel" bit for bit, and the claim
of the feature end to end — an image's restoration does not depend on the batch it travels in."""
import pytest
import torch

pytestmark = pytest.mark.gpu

USED = [50, 100, 150, 200]
# edtr_normal_fill vs the fp64 restatement.  The uniforms are identical bits on both sides; what differs is fp32 ln / sqrt / sincos:
# a few ulp of r <= 5.77 (about 2e-6) plus an angle error of at most 2 pi 2^-24 times r (about 2.2e-6) — under 5e-6, gated at twice that.
FILL_TOL = 1e-5


def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def fill(source, shape, purpose, draw=0):
    from edtr_amd import ops
    out = torch.full(shape, float("nan"), dtype=torch.float32, device="cuda:0")
    ops.launch(ops.make_normal_fill(out=out, source=source, purpose=purpose, draw=draw))
    torch.cuda.synchronize()
    return out


def _schedule(steps):
    from edtr_amd.diffusion import Diffusion
    from edtr_amd.sampler import SpacedSampler
    sampler = SpacedSampler(Diffusion(linear_start=0.00085, linear_end=0.0120, timesteps=1000).betas)
    sampler.make_schedule(steps, USED if steps == 4 else None)
    return sampler


@pytest.mark.parametrize("hw", [8, 64])
@pytest.mark.parametrize("draw", [0, 49])
@pytest.mark.parametrize("purpose", [0, 1, 2, 3])
def test_normal_fill_matches_the_host_reference(purpose, draw, hw):
    from edtr_amd import rng
    dev()
    src = rng.NoiseSource(0x1234_5678_9ABC_DEF0, [5, 0, 4_000_000_000])
    got = fill(src, (3, 4, hw, hw), purpose, draw).double().cpu().reshape(3, -1)
    want = torch.from_numpy(rng.normal_reference(src.seed, src.image_ids, purpose, draw, 4 * hw * hw))
    err = float((got - want).abs().max())
    print(f"\n[normal_fill purpose {purpose} draw {draw} {hw}x{hw}] max abs err {err:.2e}, max |z| {float(got.abs().max()):.2f}")
    assert torch.isfinite(got).all()
    assert err <= FILL_TOL


def test_fill_is_independent_of_position_and_batch():
    from edtr_amd import rng
    dev()
    for purpose, draw in ((rng.PURPOSE_STEP, 3), (rng.PURPOSE_X_T, 0)):
        five = fill(rng.NoiseSource(77, [3, 17, 9, 0, 2]), (5, 4, 32, 32), purpose, draw)
        one = fill(rng.NoiseSource(77, [17]), (1, 4, 32, 32), purpose, draw)
        assert torch.equal(five[1:2], one)
        assert not torch.equal(five[0:1], one)
    # image_ids == NULL: image_id_base + b (the C ABI's contiguous form) is the same stream
    from edtr_amd import lib, ops
    out = torch.empty((3, 64), dtype=torch.float32, device="cuda:0")
    lib.check(lib.load().edtr_normal_fill(out.data_ptr(), 3, 64, 77, None, 15, rng.PURPOSE_STEP, 3, ops.stream_ptr()), "normal_fill")
    torch.cuda.synchronize()
    assert torch.equal(out, fill(rng.NoiseSource.for_shard(77, 15, 3), (3, 64), rng.PURPOSE_STEP, 3))


def test_q_sample_rng_equals_fill_then_q_sample():
    from edtr_amd import rng
    from edtr_amd.diffusion import Diffusion
    d = dev()
    diffusion = Diffusion(linear_start=0.00085, linear_end=0.0120, timesteps=1000).to(d)
    src = rng.NoiseSource(2024, [9, 4_000_000_000, 1])
    x = rnd((3, 4, 16, 24), 1).to(d)
    noise = fill(src, tuple(x.shape), rng.PURPOSE_Q_SAMPLE)
    for t in (torch.tensor([200, 0, 999]), torch.full((3,), 200, dtype=torch.int64)):
        for tt in (t.to(d), t):                        # device t and host t
            want = diffusion.q_sample(x, t.to(d), noise)
            got = diffusion.q_sample(x, tt, src)
            torch.cuda.synchronize()
            assert torch.equal(got, want)
    assert not torch.equal(diffusion.q_sample(x, t, rng.NoiseSource(2025, src.image_ids)), want)
    with pytest.raises(ValueError):
        diffusion.q_sample(x, t, rng.NoiseSource(1, [0, 1]))             # two ids for a batch of three


@pytest.mark.parametrize("steps", [4, 50])
def test_sampler_update_rng_equals_fill_then_update_on_every_row(steps):
    """Both fused forms against the tensor-noise kernels fed with edtr_normal_fill's output, every row of the table (the sigma = 0
    row included), x_prev and pred_x0 bit for bit; and through p_sample (host index and device index)."""
    from edtr_amd import ops, rng
    d = dev()
    sampler = _schedule(steps).to(d)
    src = rng.NoiseSource(31337, [6, 2, 4_000_000_000])
    x, eps = (rnd((3, 4, 16, 16), s).to(d) for s in (1, 2))
    table = sampler._coef_table(d)
    assert table.shape[0] == steps and float(table[0, 4]) == 0.0 and float(table[1, 4]) > 0.0
    for row in range(steps):
        noise = fill(src, tuple(x.shape), rng.PURPOSE_STEP, row)
        want = torch.empty_like(x), torch.empty_like(x)
        ops.launch(ops.make_sampler_update(x=x, eps=eps, noise=noise, coefs=sampler._coefs(row), x_prev=want[0], pred_x0=want[1], n=x.numel()))
        got = torch.empty_like(x), torch.empty_like(x)
        ops.launch(ops.make_sampler_update_rng(x=x, eps=eps, source=src, draw=row, coefs=sampler._coefs(row), x_prev=got[0], pred_x0=got[1]))
        idx = torch.full((3,), row, dtype=torch.int64, device=d)
        want_i = torch.empty_like(x), torch.empty_like(x)
        ops.launch(ops.make_sampler_update_indexed(x=x, eps=eps, noise=noise, index=idx, coefs=table, x_prev=want_i[0], pred_x0=want_i[1]))
        got_i = torch.empty_like(x), torch.empty_like(x)
        ops.launch(ops.make_sampler_update_indexed_rng(x=x, eps=eps, source=src, index=idx, coefs=table, x_prev=got_i[0], pred_x0=got_i[1]))
        a = sampler.p_sample(lambda *_: eps, x, None, row, None, None, 1.0, src)
        b = sampler.p_sample(lambda *_: eps, x, None, idx, None, None, 1.0, noise_source=src)
        torch.cuda.synchronize()
        for name, g in (("scalar", got), ("indexed", got_i), ("p_sample int", a), ("p_sample device index", b)):
            assert torch.equal(g[0], want[0]) and torch.equal(g[1], want[1]), (name, row)
        assert torch.equal(want_i[0], want[0]) and torch.equal(want_i[1], want[1])
    # a per-image index: every image takes its own coefficient row AND its own draw
    idx = torch.tensor([steps - 1, 0, 1], dtype=torch.int64, device=d)
    got_i = torch.empty_like(x), torch.empty_like(x)
    ops.launch(ops.make_sampler_update_indexed_rng(x=x, eps=eps, source=src, index=idx, coefs=table, x_prev=got_i[0], pred_x0=got_i[1]))
    for b, row in enumerate(idx.tolist()):
        one = rng.NoiseSource(src.seed, [src.image_ids[b]])
        w = torch.empty_like(x[b:b + 1]), torch.empty_like(x[b:b + 1])
        ops.launch(ops.make_sampler_update_rng(x=x[b:b + 1].contiguous(), eps=eps[b:b + 1].contiguous(), source=one, draw=row,
                                               coefs=sampler._coefs(row), x_prev=w[0], pred_x0=w[1]))
        torch.cuda.synchronize()
        assert torch.equal(got_i[0][b:b + 1], w[0]) and torch.equal(got_i[1][b:b + 1], w[1])


def test_gaussian_sample_rng_equals_fill_then_gaussian_sample():
    from edtr_amd import ops, rng
    d = dev()
    src = rng.NoiseSource(5, [4_000_000_000, 3, 8, 1])
    for H, W in ((16, 24), (3, 5)):                   # (HW % 4 != 0: a group of four straddles two channels)
        B, C, HW, ld = 4, 4, H * W, 8
        mom = rnd((B * HW, ld), 5, 2.0)
        mom[:, 4:] *= 12.0                            # exercise the clamp(-30, 20)
        mom = mom.to(d)
        noise = fill(src, (B, C, H, W), rng.PURPOSE_VAE)
        want, got = (torch.empty((B, C, H, W), dtype=torch.float32, device=d) for _ in range(2))
        ops.launch(ops.make_gaussian_sample(moments=mom, ld=ld, noise=noise, out=want, B=B, C=C, HW=HW, scale=0.18215))
        ops.launch(ops.make_gaussian_sample_rng(moments=mom, ld=ld, source=src, out=got, B=B, C=C, HW=HW, scale=0.18215))
        torch.cuda.synchronize()
        assert torch.isfinite(got).all()
        assert torch.equal(got, want)


def test_vae_encode_with_a_noise_source():
    """vae_encode(sample=True, noise_source=...) = the posterior sample with the purpose-3 stream: equal bits on a second call,
    equal to the engine fed with the fill by hand, independent of torch's generator, different from another seed."""
    from edtr_amd import rng, synth
    from edtr_amd.testing import build_synthetic_cldm
    d = dev()
    cldm = build_synthetic_cldm(synth.tiny_config(), d, dtype=torch.float16)
    img = synth.synth_input("vsample:img", (2, 3, 64, 96), -1.0, 1.0).to(d)
    src = rng.NoiseSource(8, [40, 2])
    torch.manual_seed(1)
    a = cldm.vae_encode(img, noise_source=src)
    torch.manual_seed(2)
    b = cldm.vae_encode(img, sample=True, noise_source=src)
    eng = cldm.vae_engine("encode", 2, 64, 96, 0, sample=True)
    c = eng.run(img, fill(src, tuple(eng.out.shape), rng.PURPOSE_VAE)).clone()
    other = cldm.vae_encode(img, noise_source=rng.NoiseSource(9, [40, 2]))
    torch.cuda.synchronize()
    assert torch.isfinite(a).all()
    assert torch.equal(a, b) and torch.equal(a, c) and not torch.equal(a, other)
    assert not torch.equal(a, cldm.vae_encode(img, sample=False))


_SD21 = {}


def _sd21(precision, dtype):
    """The SD-2.1-width synthetic model of test_gpu_e2e's batch-invariance test, built once per precision for this file (the
    caller has set EDTR_AMD_BATCH_INVARIANT=1 before the first engine is built)."""
    from edtr_amd import synth
    from edtr_amd.diffusion import Diffusion
    from edtr_amd.sampler import SpacedSampler
    from edtr_amd.testing import build_synthetic_cldm
    d = torch.device("cuda:0")
    if precision not in _SD21:
        cldm = build_synthetic_cldm(synth.sd21_config(), d, dtype, precision=precision)
        cldm.clip.set_embedding(synth.synth_normal("inv:c_txt", (1, 77, 1024)).to(d))
        _SD21[precision] = cldm
    diffusion = Diffusion(linear_start=0.00085, linear_end=0.0120, timesteps=1000).to(d)
    return _SD21[precision], diffusion, SpacedSampler(diffusion.betas)


@pytest.mark.parametrize("precision,dtype", [("fast", torch.bfloat16), ("mixed", None)])
def test_seeded_restoration_is_bit_exact_across_batch_compositions(monkeypatch, precision, dtype):
    """The setup of test_gpu_e2e.py::test_batch_invariant_mode_is_bit_exact_across_batch_sizes WITHOUT injected noise: q_sample and
    the sampler get NoiseSource(seed, ids).  Image id 3 restored in a batch of five, alone, and first in a batch of two gives equal
    latents and images; another seed gives another latent; the same seed twice gives the same bits."""
    from edtr_amd import rng, synth
    d = dev()
    monkeypatch.setenv("EDTR_AMD_BATCH_INVARIANT", "1")
    cldm, diffusion, sampler = _sd21(precision, dtype)
    B, S = 5, 256
    pre = synth.synth_input("inv:pre_res", (B, 3, S, S), 0.0, 1.0).to(d)
    c_txt = synth.synth_normal("inv:c_txt", (1, 77, 1024)).to(d)

    def run(sel, seed=11):
        n = len(sel)
        src = rng.NoiseSource(seed, sel)
        z_pre = cldm.vae_encode(pre[sel] * 2 - 1, sample=False)
        x_T = diffusion.q_sample(z_pre, torch.full((n,), 200, dtype=torch.int64), src)
        z = sampler.manual_sample_with_timesteps(model=cldm, device=d, x_T=x_T, steps=4, used_timesteps=USED, batch_size=n,
                                                 cond={"c_txt": c_txt.expand(n, -1, -1).contiguous(), "c_img": z_pre},
                                                 uncond=None, cfg_scale=1.0, progress=False, noise_source=src)
        return z, cldm.vae_decode(z)

    z5, img5 = run([0, 1, 2, 3, 4])
    z1, img1 = run([3])
    z2, img2 = run([3, 0])
    z1b, img1b = run([3])
    z1s, _ = run([3], seed=12)
    assert torch.isfinite(img5).all()
    assert torch.equal(z5[3:4], z1) and torch.equal(img5[3:4], img1)
    assert torch.equal(z2[0:1], z1) and torch.equal(img2[0:1], img1)
    assert torch.equal(z1b, z1) and torch.equal(img1b, img1)
    assert not torch.equal(z1s, z1)


def test_restore_dataset_seeded_is_independent_of_batch_size(monkeypatch):
    """restore_dataset(seed=11) over 6 images with batch_size 1, 4 and 6 (invariant mode): the outputs are equal image by image.
    seed=None still runs."""
    from edtr_amd import evalutil, synth
    dev()
    monkeypatch.setenv("EDTR_AMD_BATCH_INVARIANT", "1")
    cldm, diffusion, sampler = _sd21("fast", torch.bfloat16)
    imgs = [synth.synth_input(f"rngdrv:img{i}", (3, 256, 256), 0.0, 1.0) for i in range(6)]
    runs = [evalutil.restore_dataset(cldm, diffusion, sampler, imgs, img_size=256, batch_size=bs, seed=11)[0] for bs in (1, 4, 6)]
    assert all(len(r) == 6 for r in runs)
    for k in range(6):
        assert torch.isfinite(runs[0][k]).all()
        assert torch.equal(runs[0][k], runs[1][k]) and torch.equal(runs[0][k], runs[2][k]), k
    assert not torch.equal(runs[0][0], evalutil.restore_dataset(cldm, diffusion, sampler, imgs[:1], img_size=256, batch_size=1, seed=12)[0][0])
    outs, _ = evalutil.restore_dataset(cldm, diffusion, sampler, imgs[:2], img_size=256, batch_size=2)       # the default path is alive
    assert len(outs) == 2 and all(torch.isfinite(o).all() for o in outs)


def test_seeded_loop_makes_no_torch_randn_call(monkeypatch):
    from edtr_amd import rng, synth
    from edtr_amd.diffusion import Diffusion
    from edtr_amd.sampler import SpacedSampler
    from edtr_amd.testing import build_synthetic_cldm
    d = dev()
    cfg = synth.tiny_config()
    cldm = build_synthetic_cldm(cfg, d, torch.float16)
    diffusion = Diffusion(linear_start=0.00085, linear_end=0.0120, timesteps=1000).to(d)
    sampler = SpacedSampler(diffusion.betas)
    B, h = 2, 16
    src = rng.NoiseSource(3, [10, 11])
    z_pre = synth.synth_normal("rng:z_pre", (B, 4, h, h)).to(d)
    cond = {"c_txt": synth.synth_input("rng:c_txt", (B, 77, cfg["unet_cfg"]["context_dim"]), -1.0, 1.0).to(d), "c_img": z_pre}

    def boom(*a, **k):
        raise AssertionError("torch.randn* called in the seeded loop")

    monkeypatch.setattr(torch, "randn_like", boom)
    monkeypatch.setattr(torch, "randn", boom)
    x_T = diffusion.q_sample(z_pre, torch.full((B,), 200, dtype=torch.int64, device=d), src)
    z = sampler.manual_sample_with_timesteps(model=cldm, device=d, x_T=x_T, steps=4, used_timesteps=USED, batch_size=B, cond=cond,
                                             uncond=None, cfg_scale=1.0, progress=False, noise_source=src)
    torch.cuda.synchronize()
    assert torch.isfinite(z).all()
    with pytest.raises(AssertionError):                 # and the unseeded loop does draw from torch
        sampler.manual_sample_with_timesteps(model=cldm, device=d, x_T=x_T, steps=4, used_timesteps=USED, batch_size=B, cond=cond,
                                             uncond=None, cfg_scale=1.0, progress=False)


def test_sample_50_steps_from_seeded_x_T():
    from edtr_amd import rng, synth
    from edtr_amd.diffusion import Diffusion
    from edtr_amd.sampler import SpacedSampler
    from edtr_amd.testing import build_synthetic_cldm
    d = dev()
    cfg = synth.tiny_config()
    cldm = build_synthetic_cldm(cfg, d, torch.float16)
    sampler = SpacedSampler(Diffusion(linear_start=0.00085, linear_end=0.0120, timesteps=1000).betas)
    B, h = 2, 16
    src = rng.NoiseSource(21, [1000, 7])
    cond = {"c_txt": synth.synth_input("rng:c_txt", (B, 77, cfg["unet_cfg"]["context_dim"]), -1.0, 1.0).to(d),
            "c_img": synth.synth_normal("rng:z_pre", (B, 4, h, h)).to(d)}

    def run(**kw):
        return sampler.sample(model=cldm, device=d, steps=50, batch_size=B, x_size=(4, h, h), cond=cond, uncond=None, cfg_scale=1.0,
                              progress=False, noise_source=src, **kw)

    a, b = run(x_T=None), run(x_T=None)
    c = run(x_T=fill(src, (B, 4, h, h), rng.PURPOSE_X_T))
    torch.cuda.synchronize()
    assert torch.isfinite(a).all()
    assert torch.equal(a, b) and torch.equal(a, c)


def test_bad_arguments_answer_the_documented_codes_and_launch_nothing():
    from edtr_amd import lib, ops
    d = dev()
    L = lib.load()
    s = ops.stream_ptr()
    x = torch.zeros((2, 64), dtype=torch.float32, device=d)
    eps, xp, p0 = torch.zeros_like(x), torch.full_like(x, 7.0), torch.full_like(x, 7.0)
    idx = torch.zeros(2, dtype=torch.int64, device=d)
    coefs = torch.zeros((4, 5), dtype=torch.float32, device=d)
    tab = torch.ones(10, dtype=torch.float32, device=d)
    P = lambda t: t.data_ptr()
    E_NULL, E_SHAPE, E_ALIGN, E_DTYPE = -1, -2, -3, -4
    assert L.edtr_normal_fill(None, 2, 64, 1, None, 0, 1, 0, s) == E_NULL
    assert L.edtr_normal_fill(P(xp), 2, 62, 1, None, 0, 1, 0, s) == E_ALIGN            # per_image % 4
    assert L.edtr_normal_fill(P(xp) + 4, 2, 60, 1, None, 0, 1, 0, s) == E_ALIGN        # 16-byte rule
    assert L.edtr_normal_fill(P(xp), 2, 64, 1, None, 0, 4, 0, s) == E_DTYPE            # unknown purpose
    assert L.edtr_normal_fill(P(xp), 0, 64, 1, None, 0, 1, 0, s) == E_SHAPE
    assert L.edtr_normal_fill(P(xp), 2, 64, 1, None, (1 << 32) - 1, 1, 0, s) == E_SHAPE   # image_id_base + B > 2^32
    assert L.edtr_normal_fill(P(xp), 2, 64, 1, None, 0, 1, -1, s) == E_SHAPE
    assert L.edtr_q_sample_rng(P(x), P(idx), P(tab), P(tab), 10, None, 2, 64, 1, None, 0, s) == E_NULL
    assert L.edtr_q_sample_rng(P(x), None, P(tab), P(tab), 10, P(xp), 2, 64, 1, None, 0, s) == E_NULL
    assert L.edtr_q_sample_rng(P(x), P(idx), P(tab), P(tab), 10, P(xp), 2, 63, 1, None, 0, s) == E_ALIGN
    assert L.edtr_sampler_update_rng(P(x), P(eps), 1.0, 0.0, 1.0, 0.0, 0.0, None, P(p0), 2, 64, 1, None, 0, 0, s) == E_NULL
    assert L.edtr_sampler_update_rng(P(x), P(eps), 1.0, 0.0, 1.0, 0.0, 0.0, P(xp), P(p0), 2, 66, 1, None, 0, 0, s) == E_ALIGN
    assert L.edtr_sampler_update_indexed_rng(P(x), P(eps), P(idx), None, 4, P(xp), P(p0), 2, 64, 1, None, 0, s) == E_NULL      # NULL coefs
    assert L.edtr_sampler_update_indexed_rng(P(x), P(eps), None, P(coefs), 4, P(xp), P(p0), 2, 64, 1, None, 0, s) == E_NULL
    assert L.edtr_sampler_update_indexed_rng(P(x), P(eps), P(idx), P(coefs), 4, P(xp), P(p0), 2, 61, 1, None, 0, s) == E_ALIGN
    assert L.edtr_sampler_update_indexed_rng(P(x), P(eps), P(idx), P(coefs), 0, P(xp), P(p0), 2, 64, 1, None, 0, s) == E_SHAPE
    assert L.edtr_gaussian_sample_rng(None, 8, P(xp), 2, 4, 16, 1.0, 1, None, 0, s) == E_NULL
    assert L.edtr_gaussian_sample_rng(P(x), 8, P(xp), 2, 3, 5, 1.0, 1, None, 0, s) == E_ALIGN      # C * HW = 15
    assert L.edtr_gaussian_sample_rng(P(x), 7, P(xp), 2, 4, 16, 1.0, 1, None, 0, s) == E_SHAPE     # ld < 2 C
    torch.cuda.synchronize()
    assert bool((xp == 7.0).all()) and bool((p0 == 7.0).all())           # nothing was launched
