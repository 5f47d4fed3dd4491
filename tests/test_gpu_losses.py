"""The training losses on the device (-m gpu): edtr_l1_forward / edtr_l1_backward / edtr_cls_ce_forward / edtr_cls_ce_backward
(csrc/losses.hip) through `edtr_amd.losses` against the numpy restatements — the L1 bit for bit, the cross-entropy within the bound
tests/losses_cases.py derives against torch's fp64 chain; guarded buffers, grid independence, autograd, the training classifier and the
refusals."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import losses_cases as K
from edtr_amd import cls, losses, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
TORCH = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
GUARD = 64          # elements on each side of a guarded buffer


def guarded(n, dtype, offset=0):
    """(buffer, its inner n elements starting ``offset`` elements past the guard): NaN everywhere"""
    buf = torch.full((n + offset + 2 * GUARD,), float("nan"), dtype=dtype, device=DEV)
    return buf, buf[GUARD + offset:GUARD + offset + n]


def guards_intact(buf, n, offset=0):
    return bool(torch.isnan(buf[:GUARD + offset]).all()) and bool(torch.isnan(buf[GUARD + offset + n:]).all())


def placed(x, dtype, offset):
    """the host array on the device in ``dtype``, ``offset`` elements into its buffer (a view: its pointer is not aligned to a vector)"""
    buf = torch.zeros(x.size + offset, dtype=dtype, device=DEV)
    buf[offset:] = torch.from_numpy(np.array(x)).to(DEV).to(dtype)
    return buf[offset:]


@functools.lru_cache(maxsize=None)
def l1_launched(name, max_blocks=0, run=0):
    """the three launches on guarded, NaN-filled buffers and a workspace of 0xA5: dict of host arrays (``run`` tells repeated calls apart)"""
    case = K.L1_BY_NAME[name]
    pairs = [(placed(a, TORCH[p["dtype"]], p["offset"]), placed(b, TORCH[p["dtype"]], p["offset"])) for (a, b), p in zip(K.l1_inputs(name), case["pairs"])]
    k = len(pairs)
    loss = torch.full((), float("nan"), dtype=torch.float32, device=DEV)
    terms_buf, terms = guarded(k, torch.float32)
    workspace = torch.full((ops.l1_workspace([p["n"] for p in case["pairs"]]),), 0xA5, dtype=torch.uint8, device=DEV)    # (never zeroed: nothing relies on a memset)
    ops.launch(ops.make_l1_forward(pairs=pairs, weights=case["weights"], workspace=workspace, loss=loss, terms=terms, max_blocks=max_blocks))
    bufs_a = [guarded(p["n"], TORCH[p["dtype"]], p["offset"]) if p["need_a"] else (None, None) for p in case["pairs"]]
    bufs_b = [guarded(p["n"], TORCH[p["dtype"]], p["offset"]) if p["need_b"] else (None, None) for p in case["pairs"]]
    g = torch.tensor(K.GRAD_LOSS, dtype=torch.float32, device=DEV)
    ops.launch(ops.make_l1_backward(pairs=pairs, weights=case["weights"], grad_loss=g, grads_a=[v for _, v in bufs_a], grads_b=[v for _, v in bufs_b],
                                    max_blocks=max_blocks))
    torch.cuda.synchronize()
    intact = guards_intact(terms_buf, k) and all(guards_intact(buf, p["n"], p["offset"]) for bufs in (bufs_a, bufs_b)
                                                  for (buf, _), p in zip(bufs, case["pairs"]) if buf is not None)
    host = lambda v: None if v is None else v.float().cpu().numpy()
    return dict(loss=loss.cpu().numpy(), terms=terms.cpu().numpy(), grad_a=[host(v) for _, v in bufs_a], grad_b=[host(v) for _, v in bufs_b], guards=intact)


@pytest.mark.parametrize("name", K.L1_IDS)
def test_l1_launches_equal_the_restatement_bit_for_bit(name):
    case = K.L1_BY_NAME[name]
    got = l1_launched(name)
    pairs, dts = K.l1_inputs(name), K.l1_dtypes(case)
    loss, terms = losses.l1_mean_reference(pairs, case["weights"], dts)
    ga, gb = losses.l1_mean_backward_reference(pairs, case["weights"], K.GRAD_LOSS, dts)
    assert got["guards"], "a guard word was written"
    assert K.same_bits(got["loss"], loss) and K.same_bits(got["terms"], terms), (got["loss"], loss, got["terms"], terms)
    r = K.l1_ratio(name, got["loss"], got["terms"])
    print(f"{name}: launch error / bound against the fp64 chain  loss {r[0]:.3g}  terms {r[1]:.3g}")
    assert max(r) <= 1.0
    want_a, want_b = K.l1_expected_grads(name)
    for k, p in enumerate(case["pairs"]):
        for side, need, mine, rule, again in (("a", p["need_a"], got["grad_a"][k], want_a[k], ga[k]), ("b", p["need_b"], got["grad_b"][k], want_b[k], gb[k])):
            if not need:
                assert mine is None
                continue
            assert not np.isnan(mine).any(), f"pair {k} grad_{side}: a word was not written"        # (the buffers were NaN)
            assert K.same_bits(mine, again) and K.same_bits(mine, rule), f"pair {k} grad_{side}"


@pytest.mark.parametrize("name", ["n4097", "fold", "views", "mixed5", "optional"])
def test_l1_two_calls_and_every_grid_give_the_same_bits(name):
    first = l1_launched(name)
    for other in (l1_launched(name, 0, 1), l1_launched(name, 1), l1_launched(name, 2)):
        assert first["loss"].tobytes() == other["loss"].tobytes() and first["terms"].tobytes() == other["terms"].tobytes() and other["guards"]
        for side in ("grad_a", "grad_b"):
            for x, y in zip(first[side], other[side]):
                assert (x is None and y is None) or x.tobytes() == y.tobytes()


def test_l1_order_depends_on_n_alone_on_the_device():
    """the same values as fp32 and as fp16, aligned and one element into their buffers, alone and last in a list: one term, the same bits"""
    (a, b), = K.l1_inputs("f16_odd")
    extra = (torch.rand(777, device=DEV), torch.rand(777, device=DEV))
    seen = []
    for dtype in (torch.float32, torch.float16):
        for offset in (0, 1):
            pair = (placed(a, dtype, offset), placed(b, dtype, offset))
            seen.append(losses.l1_mean([pair], return_terms=True)[1][0].item())
            seen.append(losses.l1_mean([extra, pair], [3.0, 1.0], return_terms=True)[1][1].item())
    assert len(set(np.float32(v).tobytes() for v in seen)) == 1 and seen[0] == float(l1_launched("f16_odd")["terms"][0])


def test_l1_autograd_is_the_backward_launch_and_runs_only_when_asked():
    case = K.L1_BY_NAME["optional"]
    direct = l1_launched("optional")
    dev = [(torch.from_numpy(np.array(a)).to(DEV), torch.from_numpy(np.array(b)).to(DEV)) for a, b in K.l1_inputs("optional")]
    for (a, b), p in zip(dev, case["pairs"]):
        a.requires_grad_(p["need_a"]), b.requires_grad_(p["need_b"])
    loss, terms = losses.l1_mean(dev, case["weights"], return_terms=True)
    assert loss.requires_grad and not terms.requires_grad and loss.shape == () and loss.dtype == torch.float32
    (K.GRAD_LOSS * loss).backward()
    assert K.same_bits(loss.item(), direct["loss"]) and K.same_bits(terms.cpu().numpy(), direct["terms"])
    for k, ((a, b), p) in enumerate(zip(dev, case["pairs"])):           # a gradient exactly where one was asked for, the launch's bits
        for t, need, want in ((a, p["need_a"], direct["grad_a"][k]), (b, p["need_b"], direct["grad_b"][k])):
            assert (t.grad is not None) == need
            if need:
                assert K.same_bits(t.grad.cpu().numpy(), want)
    by_hand = losses.l1_mean_backward([(a.detach(), b.detach()) for a, b in dev], case["weights"], K.GRAD_LOSS,
                                      [p["need_a"] for p in case["pairs"]], [p["need_b"] for p in case["pairs"]])
    assert by_hand[0][1] is None and by_hand[0][2] is None and by_hand[1][2] is None and K.same_bits(by_hand[1][1].cpu().numpy(), direct["grad_b"][1])
    # grad mode off, or operands that do not require grad: the forward alone
    with torch.no_grad():
        off = losses.l1_mean(dev, case["weights"])
    plain = losses.l1_mean([(a.detach(), b.detach()) for a, b in dev], case["weights"])
    assert off.grad_fn is None and not off.requires_grad and plain.grad_fn is None and not plain.requires_grad
    assert off.item() == plain.item() == loss.item()
    # feature_matching: the segmenter's and the detector's forms are l1_mean of the same pairs
    maps = ({"0": dev[0][0].detach(), "1": dev[1][0].detach(), "pool": dev[2][0].detach()}, {"0": dev[0][1].detach(), "1": dev[1][1].detach(), "pool": dev[2][1].detach()})
    fm = losses.feature_matching(*maps, keys=("0", "1"), weights=(0.5, 0.5), weight=2.0)
    assert fm.item() == losses.l1_mean([(maps[0]["0"], maps[1]["0"]), (maps[0]["1"], maps[1]["1"])], [1.0, 1.0]).item()
    assert losses.feature_matching(maps[0]["0"], maps[1]["0"], weight=0.5).item() == losses.feature_matching(*maps, keys=("0",), weight=0.5).item()


@functools.lru_cache(maxsize=None)
def ce_launched(name, run=0):
    case = K.CE_BY_NAME[name]
    x, t = K.ce_inputs(name)
    B, C = x.shape
    logits = torch.from_numpy(np.array(x)).to(DEV).to(TORCH[case["dtype"]])
    labels = torch.from_numpy(np.array(t)).to(DEV).to(torch.int32)
    lse_buf, lse = guarded(B, torch.float32)
    grad_buf, grad = guarded(B * C, logits.dtype)
    loss = torch.full((), float("nan"), dtype=torch.float32, device=DEV)
    counts = torch.full((2,), -1, dtype=torch.int64, device=DEV)
    workspace = torch.full((8 * B,), 0xA5, dtype=torch.uint8, device=DEV)
    ops.launch(ops.make_cls_ce_forward(logits=logits, labels=labels, lse=lse, workspace=workspace, loss=loss, counts=counts, ignore_index=K.IGNORE))
    g = torch.tensor(K.GRAD_LOSS, dtype=torch.float32, device=DEV)
    ops.launch(ops.make_cls_ce_backward(logits=logits, labels=labels, lse=lse, counts=counts, grad_loss=g, grad=grad.view(B, C), ignore_index=K.IGNORE))
    torch.cuda.synchronize()
    return dict(loss=loss.cpu().numpy(), lse=lse.cpu().numpy(), grad=grad.view(B, C).float().cpu().numpy(), counts=counts.cpu().tolist(),
                guards=guards_intact(lse_buf, B) and guards_intact(grad_buf, B * C))


@pytest.mark.parametrize("name", K.CE_IDS)
def test_ce_launches_against_the_restatement_and_the_fp64_chain(name):
    case = K.CE_BY_NAME[name]
    x, t = K.ce_inputs(name)
    got = ce_launched(name)
    loss, lse, count, bad = losses.cross_entropy_reference(x, t, K.IGNORE, case["dtype"])
    grad = losses.cross_entropy_backward_reference(x, t, lse, count, K.GRAD_LOSS, K.IGNORE, case["dtype"])
    assert got["counts"] == [count, bad] and got["guards"], "counts, or a guard word was written"
    assert not np.isnan(got["lse"]).any() and not np.isnan(got["grad"]).any()          # every inner word is written (the buffers were NaN)
    assert np.isnan(got["loss"]) == np.isnan(loss)
    keep = K.ce_keep(case, t)
    assert not got["grad"][~keep].any() and not np.signbit(got["grad"][~keep]).any()    # ignored and bad rows: +0.0, written
    r = K.ce_ratios(name, got["loss"], got["lse"], got["grad"])
    dist = (abs(float(got["loss"]) - float(loss)) if count else 0.0, float(np.abs(got["lse"] - lse).max()), float(np.abs(got["grad"] - grad).max()))
    print(f"{name}: launch error / bound  loss {r[0]:.3g}  lse {r[1]:.3g}  grad {r[2]:.3g};  launch - restatement  loss {dist[0]:.3g}  lse {dist[1]:.3g}  "
          f"grad {dist[2]:.3g} (largest |grad| {np.abs(grad).max():.3g})")
    assert max(r) <= 1.0
    if name == "one_class":
        assert got["loss"] == 0.0 and not got["grad"].any() and not np.signbit(got["grad"]).any()
    if count == 0:
        assert not got["grad"].any()
    again = ce_launched(name, 1)
    assert all(got[k].tobytes() == again[k].tobytes() for k in ("loss", "lse", "grad")) and got["counts"] == again["counts"]


def test_ce_autograd_is_the_backward_launch_and_runs_only_when_asked():
    x, t = K.ce_inputs("ignored_rows")
    direct = ce_launched("ignored_rows")
    labels = torch.from_numpy(np.array(t)).to(DEV)
    logits = torch.from_numpy(np.array(x)).to(DEV).requires_grad_(True)
    loss, counts = losses.cross_entropy(logits, labels, return_counts=True)
    assert loss.requires_grad and not counts.requires_grad and loss.shape == () and loss.dtype == torch.float32
    (K.GRAD_LOSS * loss).backward()
    assert logits.grad.cpu().numpy().tobytes() == direct["grad"].tobytes() and loss.item() == float(direct["loss"]) and counts.tolist() == direct["counts"]
    l2, c2, lse = losses.cross_entropy(logits.detach(), labels, return_saved=True)
    by_hand = losses.cross_entropy_backward(logits.detach(), labels, lse, c2, K.GRAD_LOSS)
    assert l2.item() == loss.item() and by_hand.cpu().numpy().tobytes() == direct["grad"].tobytes()
    with torch.no_grad():
        off = losses.cross_entropy(logits, labels)
    plain = losses.cross_entropy(logits.detach(), labels)
    assert off.grad_fn is None and not off.requires_grad and plain.grad_fn is None and not plain.requires_grad
    assert off.item() == plain.item() == loss.item()


class Stub(torch.nn.Module):
    """two convolutions and a linear layer, with return_feat"""
    def __init__(self):
        super().__init__()
        self.conv1, self.conv2 = torch.nn.Conv2d(3, 8, 3, stride=2, padding=1), torch.nn.Conv2d(8, 8, 3, stride=2, padding=1)
        self.fc = torch.nn.Linear(8, 5)

    def forward(self, x, return_feat=False):
        feat = self.conv2(torch.relu(self.conv1(x)))
        pred = self.fc(feat.mean(dim=(2, 3)))
        return (pred, feat) if return_feat else pred


def test_training_classifier_hands_the_launches_gradients_to_the_stub():
    """One step through `cls.assemble_training_classifier`.  The gradients that reach the stub's logits and features are the launches'
    (bit for bit those of the backward wrappers, and within the derived bounds of the fp64 chains); the parameter gradients are
    torch's own backward of the stub from those output gradients: run twice, they may differ only by the rounding of that backward,
    2 u n_ops |J|^T |g| with |J|^T the stub's backward with every weight and activation replaced by its absolute value (the ReLU mask
    kept) and n_ops = 2 * 16 * 16 * 72 + 64 + 5 + 8, the longest sum a parameter gradient is."""
    torch.manual_seed(5)
    student, teacher = Stub().to(DEV), Stub().to(DEV)
    params = list(student.parameters())
    images, gts = torch.rand(4, 3, 32, 32, device=DEV), torch.rand(4, 3, 32, 32, device=DEV)
    labels = torch.tensor([1, 4, -100, 0], device=DEV)
    w_ce, w_fm = 0.75, 2.0
    train_step = cls.assemble_training_classifier(student, teacher, weight_ce=w_ce, weight_fm=w_fm)
    with torch.no_grad():                   # (train_step turns grad mode on itself)
        out, (pred, feat) = train_step(images, labels, gts)
    assert set(out) == {"ce", "fm"} and out["ce"].requires_grad and out["fm"].requires_grad and pred.shape == (4, 5) and feat.shape == (4, 8, 8, 8)
    assert set(cls.assemble_training_classifier(student)(images, labels)[0]) == {"ce"}             # no teacher: no "fm"
    pred.retain_grad(), feat.retain_grad()
    (out["ce"] + out["fm"]).backward(retain_graph=True)
    ours = [p.grad.clone() for p in params]
    pred_grad, feat_grad = pred.grad.clone(), feat.grad.clone()            # (a later pass through the graph would add to the retained gradients)
    with torch.no_grad():
        _, feat_teacher = teacher(gts, return_feat=True)
    # the logits' gradient is the cross-entropy launch's for the upstream gradient weight_ce, the features' the L1 launch's plus the head's
    plain_ce, counts, lse = losses.cross_entropy(pred.detach(), labels, return_saved=True)
    g_pred = losses.cross_entropy_backward(pred.detach(), labels, lse, counts, w_ce)
    (g_feat,), _ = losses.l1_mean_backward([(feat.detach(), feat_teacher)], [w_fm], 1.0)
    assert torch.equal(pred_grad, g_pred)
    through_head, = torch.autograd.grad(pred, feat, grad_outputs=g_pred, retain_graph=True)
    assert torch.equal(feat_grad, g_feat + through_head)
    # ... and they meet the bounds: the fp64 chains of the same logits and features
    ce_case = K.ce_given("training_stub_ce", pred.detach().cpu().numpy(), labels.cpu().numpy())
    assert out["ce"].item() == (plain_ce * w_ce).item()
    r = K.ce_ratios(ce_case["name"], plain_ce.item(), lse.cpu().numpy(), g_pred.cpu().numpy().astype(np.float64) * (K.GRAD_LOSS / w_ce))
    l1_case = K.l1_given("training_stub_fm", [(feat.detach().cpu().numpy(), feat_teacher.cpu().numpy())], [w_fm], ["float32"])
    rule_a, _ = losses.l1_mean_backward_reference(K.l1_inputs(l1_case["name"]), [w_fm], 1.0, ["float32"])
    print(f"training stub: logits' gradient error / bound {r[2]:.3g} (loss {r[0]:.3g})")
    assert max(r) <= 1.0 and K.same_bits(g_feat.cpu().numpy().reshape(-1), rule_a[0])         # (the bound is linear in the upstream gradient)
    # the loss values against torch's chain on the same device: each side within its bound of the exact value
    theirs_ce = F.cross_entropy(pred.detach(), labels) * w_ce
    theirs_fm = F.l1_loss(feat.detach(), feat_teacher) * w_fm
    assert abs(out["ce"].item() - theirs_ce.item()) <= 2 * w_ce * K.ce_bounds(ce_case["name"])["loss"]
    assert abs(out["fm"].item() - theirs_fm.item()) <= 2 * K.l1_bounds(l1_case["name"])["loss"]
    # the parameter gradients: torch.autograd.grad of the stub from those same output gradients
    pred2, feat2 = student(images, return_feat=True)
    theirs = torch.autograd.grad([pred2, feat2], params, grad_outputs=[g_pred, g_feat])
    twin = [p.detach().abs().requires_grad_(True) for p in params]
    mask = (student.conv1(images) > 0).float().detach()
    feat_abs = F.conv2d(F.conv2d(images.abs(), twin[0], twin[1], stride=2, padding=1) * mask, twin[2], twin[3], stride=2, padding=1)
    pred_abs = F.linear(feat_abs.mean(dim=(2, 3)), twin[4], twin[5])
    n_ops = 2 * 16 * 16 * 72 + 64 + 5 + 8
    limit = torch.autograd.grad([pred_abs, feat_abs], twin, grad_outputs=[2 * K.U * n_ops * g_pred.abs(), 2 * K.U * n_ops * g_feat.abs()])
    for name, a, b, lim in zip(("conv1.w", "conv1.b", "conv2.w", "conv2.b", "fc.w", "fc.b"), ours, theirs, limit):
        diff = (a - b).abs()
        ratio = float(torch.where(diff == 0, torch.zeros_like(diff), diff / lim).max())
        print(f"{name}: |ours - torch's| / propagated bound {ratio:.3g} (largest |gradient| {float(b.abs().max()):.3g})")
        assert float(b.abs().max()) > 0 and ratio <= 1.0


def test_rejections_launch_nothing():
    from edtr_amd import lib
    h = lib.load()
    K.check_l1_rejections(h)
    K.check_ce_rejections(h)
    a, b = torch.zeros(2, 3, device=DEV), torch.zeros(2, 3, device=DEV)
    with pytest.raises(TypeError):
        losses.l1_mean([(a.double(), b.double())])
    with pytest.raises(TypeError):
        losses.l1_mean([(a, b.half())])
    with pytest.raises(ValueError):
        losses.l1_mean([(a, torch.zeros(3, 2, device=DEV))])
    with pytest.raises(ValueError):
        losses.l1_mean([(a, b)] * 9)
    with pytest.raises(ValueError):
        losses.l1_mean([(a, b)], max_blocks=-1)
    with pytest.raises(TypeError):
        losses.l1_mean([(a, b.cpu())])
    with pytest.raises(ValueError):
        losses.l1_mean_backward([(a, b)], need_a=[False], need_b=[False])
    logits, labels = torch.zeros(2, 3, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError):
        losses.cross_entropy(logits, labels, label_smoothing=0.1)
    with pytest.raises(TypeError):
        losses.cross_entropy(logits.double(), labels)
    with pytest.raises(TypeError):
        losses.cross_entropy(logits[None], labels)
    with pytest.raises(TypeError):
        losses.cross_entropy(logits, labels[:1])
    with pytest.raises(TypeError):
        losses.cross_entropy(logits, labels.float())
    with pytest.raises(RuntimeError):                                                            # a NULL pointer through the C entry: EDTR_E_NULL
        ops.launch(ops.make_l1_forward(pairs=[(a, b)], weights=[1.0], workspace=torch.zeros(8, dtype=torch.uint8, device=DEV), loss=None))
    with pytest.raises(RuntimeError):
        ops.launch(ops.make_cls_ce_forward(logits=logits, labels=labels.int(), lse=None, workspace=torch.zeros(16, dtype=torch.uint8, device=DEV),
                                           loss=torch.zeros((), device=DEV), counts=torch.zeros(2, dtype=torch.int64, device=DEV)))
