"""The segmentation loss from coarse logits on the device (-m gpu): edtr_seg_ce_forward / edtr_seg_ce_backward (csrc/seg_loss.hip) through
`labels.coarse_cross_entropy` against the numpy restatements and, within the bound tests/seg_loss_cases.py derives, torch's fp64 chain;
guarded buffers, grid independence, autograd, the training segmenter and the refusals."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import seg_loss_cases as K
from edtr_amd import labels, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
TORCH = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
GUARD = 64          # elements on each side of a guarded buffer


def guarded(shape, dtype):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(shape)


def guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


@functools.lru_cache(maxsize=None)
def launched(name, max_blocks=0, run=0):
    """the two launches on guarded, NaN-filled buffers: dict of host arrays (``run`` only tells repeated calls apart)"""
    case = K.BY_NAME[name]
    x, t = K.inputs(case)
    coarse, target = torch.from_numpy(x).to(DEV).to(TORCH[case["dtype"]]), torch.from_numpy(t).to(DEV)
    B, H, W = t.shape
    lse_buf, lse = guarded((B, H, W), torch.float32)
    grad_buf, grad = guarded(x.shape, coarse.dtype)
    loss = torch.full((), float("nan"), dtype=torch.float32, device=DEV)
    counts = torch.full((2,), -1, dtype=torch.int64, device=DEV)
    workspace = torch.full((ops.seg_ce_workspace(B, H, W),), 0xA5, dtype=torch.uint8, device=DEV)       # (never zeroed: nothing relies on a memset)
    ops.launch(ops.make_seg_ce_forward(coarse=coarse, target=target, lse=lse, workspace=workspace, loss=loss, counts=counts, max_blocks=max_blocks))
    g = torch.tensor(K.GRAD_LOSS, dtype=torch.float32, device=DEV)
    ops.launch(ops.make_seg_ce_backward(coarse=coarse, target=target, lse=lse, counts=counts, grad_loss=g, grad=grad, max_blocks=max_blocks))
    torch.cuda.synchronize()
    return dict(loss=loss.cpu().numpy(), lse=lse.cpu().numpy(), grad=grad.float().cpu().numpy(), counts=counts.cpu().tolist(),
                guards=guards_intact(lse_buf) and guards_intact(grad_buf))


@functools.lru_cache(maxsize=None)
def restated(name):
    case = K.BY_NAME[name]
    x, t = K.inputs(case)
    loss, lse, count, bad = labels.coarse_cross_entropy_reference(x, t, dtype=case["dtype"])
    return loss, lse, count, bad, labels.coarse_cross_entropy_backward_reference(x, t, lse, count, K.GRAD_LOSS, dtype=case["dtype"])


@pytest.mark.parametrize("name", K.CASE_IDS)
def test_launches_against_the_restatement_and_the_fp64_chain(name):
    got = launched(name)
    loss, lse, count, bad, grad = restated(name)
    assert got["counts"] == [count, bad]
    assert got["guards"], "a guard word was written"
    # every inner word is written (the buffers were NaN), NaNs and zeros where the restatement has them
    assert not np.isnan(got["lse"]).any() and not np.isnan(got["grad"]).any()
    assert np.isnan(got["loss"]) == np.isnan(loss)
    exact = K.reference(name)["grad"] == 0                       # unreached positions, dead images, the one-class case: +0.0, written
    assert not got["grad"][exact].any() and not np.signbit(got["grad"][exact]).any()
    if K.BY_NAME[name]["dtype"] == "float16":                   # (a sum next to half of float16's smallest subnormal may round either way)
        assert np.all(np.abs(K.reference(name)["grad"][got["grad"] == 0]) < 2.0 ** -23)
    else:
        assert np.array_equal(got["grad"] == 0, grad == 0)
    r = K.ratios(name, got["loss"], got["lse"], got["grad"])
    dist = (abs(float(got["loss"]) - float(loss)) if count else 0.0, float(np.abs(got["lse"] - lse).max()), float(np.abs(got["grad"] - grad).max()))
    print(f"{name}: launch error / bound  loss {r[0]:.3g}  lse {r[1]:.3g}  grad {r[2]:.3g};  launch - restatement  loss {dist[0]:.3g}  lse {dist[1]:.3g}  "
          f"grad {dist[2]:.3g} (largest |grad| {np.abs(grad).max():.3g})")
    assert max(r) <= 1.0
    if name == "e_one_class":
        assert got["loss"] == 0.0 and not got["grad"].any()
    if count == 0:
        assert not got["grad"].any()


@pytest.mark.parametrize("name", ["a_8x", "b_fractional_bf16", "d_memory", "f_tiles", "h_footprint"])
def test_two_calls_and_every_grid_give_the_same_bits(name):
    first, again, one = launched(name), launched(name, 0, 1), launched(name, 1)
    for other in (again, one):
        assert first["loss"].tobytes() == other["loss"].tobytes() and first["lse"].tobytes() == other["lse"].tobytes()
        assert first["grad"].tobytes() == other["grad"].tobytes() and first["counts"] == other["counts"]


def test_autograd_is_the_backward_launch_and_runs_only_when_asked():
    case = K.BY_NAME["b_fractional"]
    x, t = K.inputs(case)
    target = torch.from_numpy(t).to(DEV)
    coarse = torch.from_numpy(x).to(DEV).requires_grad_(True)
    loss, counts = labels.coarse_cross_entropy(coarse, target, return_counts=True)
    assert loss.requires_grad and not counts.requires_grad and loss.shape == () and loss.dtype == torch.float32
    (0.37 * loss).backward()
    direct = launched("b_fractional")
    assert coarse.grad.cpu().numpy().tobytes() == direct["grad"].tobytes() and loss.item() == float(direct["loss"])
    # through CoarseLogits, and the saved tensors handed to the backward by hand
    again = labels.coarse_cross_entropy(labels.CoarseLogits(coarse.detach(), (37, 50)), target)
    l2, c2, lse = labels.coarse_cross_entropy(coarse.detach(), target, return_saved=True)
    by_hand = labels.coarse_cross_entropy_backward(coarse.detach(), target, lse, c2, 0.37)
    assert again.item() == l2.item() == loss.item() and by_hand.cpu().numpy().tobytes() == direct["grad"].tobytes()
    # grad mode off, or logits that do not require grad: the forward alone
    with torch.no_grad():
        off = labels.coarse_cross_entropy(coarse, target)
    plain = labels.coarse_cross_entropy(coarse.detach(), target)
    assert off.grad_fn is None and not off.requires_grad and plain.grad_fn is None and not plain.requires_grad
    assert off.item() == plain.item() == loss.item()


def test_training_segmenter_gives_the_parameter_gradients_of_torchs_chain():
    """A two-layer stub backbone and a 1 x 1 classifier, trained one step through `assemble_training_segmenter` and through torch's
    interpolate -> cross_entropy on the same device.  Both sides run the same torch backward through the stub, on logit gradients that
    each lie within E_g (the derived bound) of the exact one: the parameter gradients differ by at most |J|^T (2 E_g), with |J|^T the
    stub's backward with every weight and activation replaced by its absolute value (the ReLU mask kept), plus the rounding of that
    backward itself on either side, 2 u n_ops |J|^T |g| with n_ops = 2 * 8 * 8 * 72 + 8: the longest sum a parameter gradient is
    (batch x positions x a 3 x 3 x 8 window of the next layer's backward, and the 8 channels of the classifier)."""
    torch.manual_seed(3)
    conv1, conv2 = torch.nn.Conv2d(3, 8, 3, stride=2, padding=1).to(DEV), torch.nn.Conv2d(8, 8, 3, stride=2, padding=1).to(DEV)
    classifier = torch.nn.Conv2d(8, 5, 1).to(DEV)
    backbone = lambda x: {"C5": conv2(torch.relu(conv1(x)))}
    params = list(conv1.parameters()) + list(conv2.parameters()) + list(classifier.parameters())
    images = torch.rand(2, 3, 32, 32, device=DEV)
    masks = torch.randint(0, 5, (2, 32, 32), dtype=torch.uint8, device=DEV)
    masks[0, :4] = 255
    train_step = labels.assemble_training_segmenter(backbone, classifier, normalize=False)
    with torch.no_grad():                   # (train_step turns grad mode on itself)
        loss, feats = train_step(images, masks)
    assert loss.requires_grad and feats["C5"].shape == (2, 8, 8, 8)
    ours = torch.autograd.grad(loss, params)
    logits = classifier(backbone(images)["C5"])
    theirs_loss = F.cross_entropy(F.interpolate(logits, size=(32, 32), mode="bilinear", align_corners=False), masks.long(), ignore_index=255)
    theirs = torch.autograd.grad(theirs_loss, params)
    case = K.given("training_stub", logits.detach().cpu().numpy(), masks.cpu().numpy())
    E = torch.from_numpy(K.bounds(case["name"])["grad"] / K.GRAD_LOSS).float().to(DEV)          # (the bound is linear in the upstream gradient)
    g = torch.from_numpy(np.abs(K.reference(case["name"])["grad"]) / K.GRAD_LOSS).float().to(DEV)
    assert abs(loss.item() - theirs_loss.item()) <= 2 * K.bounds(case["name"])["loss"]
    # |J|^T: the stub with absolute weights and inputs, the ReLU as the mask the real forward had
    twin = [p.detach().abs().requires_grad_(True) for p in params]
    mask = (conv1(images) > 0).float()
    h = F.conv2d(F.conv2d(images.abs(), twin[0], twin[1], stride=2, padding=1) * mask, twin[2], twin[3], stride=2, padding=1)
    out = F.conv2d(h, twin[4], twin[5])
    n_ops = 2 * 8 * 8 * 72 + 8
    limit = torch.autograd.grad(out, twin, grad_outputs=2 * E + 2 * K.U * n_ops * g)
    for name, a, b, lim in zip(("conv1.w", "conv1.b", "conv2.w", "conv2.b", "cls.w", "cls.b"), ours, theirs, limit):
        diff = (a - b).abs()
        ratio = float(torch.where(diff == 0, torch.zeros_like(diff), diff / lim).max())        # (a channel the ReLU never lets through: 0 / 0)
        print(f"{name}: |ours - torch's| / propagated bound {ratio:.3g} (largest |gradient| {float(b.abs().max()):.3g})")
        assert float(b.abs().max()) > 0 and ratio <= 1.0


def test_rejections_launch_nothing():
    from edtr_amd import lib
    K.check_rejections(lib.load())
    t = torch.zeros((1, 8, 8), dtype=torch.uint8, device=DEV)
    coarse = torch.zeros((1, 21, 2, 2), device=DEV)
    with pytest.raises(ValueError):
        labels.coarse_cross_entropy(torch.zeros((1, 257, 2, 2), device=DEV), t)                  # n > 256
    with pytest.raises(TypeError):
        labels.coarse_cross_entropy(torch.zeros((1, 21, 2, 4), device=DEV)[:, :, :, ::2], t)     # not contiguous
    with pytest.raises(TypeError):
        labels.coarse_cross_entropy(torch.zeros((1, 21, 2, 2), dtype=torch.float64, device=DEV), t)
    with pytest.raises(ValueError):
        labels.coarse_cross_entropy(coarse, t.long())                                            # a target of another dtype
    with pytest.raises(ValueError):
        labels.coarse_cross_entropy(coarse, torch.zeros((2, 8, 8), dtype=torch.uint8, device=DEV))      # ... of another batch
    with pytest.raises(ValueError):
        labels.coarse_cross_entropy(coarse, t, size=(8, 9))                                      # a size that is not the target's extent
    with pytest.raises(ValueError):
        labels.coarse_cross_entropy(labels.CoarseLogits(coarse, (8, 9)), t)
    with pytest.raises(RuntimeError):                                                            # a NULL pointer through the C entry: EDTR_E_NULL
        ops.launch(ops.make_seg_ce_forward(coarse=coarse, target=t, lse=None, workspace=torch.zeros(16, dtype=torch.uint8, device=DEV),
                                           loss=torch.zeros((), device=DEV), counts=torch.zeros(2, dtype=torch.int64, device=DEV)))
