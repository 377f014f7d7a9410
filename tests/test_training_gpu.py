"""The matcher's training head on the GPU (include/gatsspg_train.h, onepose_amd.training): every stage entry point and the whole
head against the fp64 oracle (tests/train_oracle.py) evaluated at the same fp32 inputs, at the shapes where tiles (128 x 64) and sums
can go wrong and over the target compositions; repeatability; impl="hip" against impl="eager"; one training step; a few Adam steps.

Bounds.  Loss: relative error <= max(1e-6, 4 x the reference's own fp32 deviation from its fp64 run on that case); 1e-6 is 16 fp32
ulps.  A gradient-like tensor (dx, dy, dS, rowsum(H), colsum(H)): max|d| / max|oracle| <= max(2e-6, 4 x the reference's deviation
of dx / dy on that case); 2e-6 is 32 ulps.  The deviations are recorded in train_golden_meta.json (tests/golden/make_train_golden.py
runs the unmodified reference on every case here in fp32 and fp64); they are 2e-8 .. 1.2e-6 except where every entry is a negative:
every term is then ~ C^3 with C ~ 1e-4 and carries three times the relative error of C, 4e-6 .. 5e-6 for the reference itself.  E, r, c:
relative 4e-6 per entry -- the fp32 MFMA dot product of two unit vectors is within 1.5e-7 of the exact one (K = 256), i.e. 2.1e-6 on
S = . / 0.07, the division rounds S (<= 14.3) by 9e-7 and expf by 1.2e-7 more."""
import json
import os

import numpy as np
import pytest
import torch

import onepose_amd
import train_oracle
from onepose_amd import _native_train, synthetic
from onepose_amd.training import MatchingLoss, SparseTarget, training_loss
from conftest import GOLDEN_DIR, load_golden

pytestmark = pytest.mark.gpu

LOSS_RTOL, GRAD_RTOL, E_RTOL = 1e-6, 2e-6, 4e-6
DEFAULT, CASES = train_oracle.DEFAULT, train_oracle.GPU_CASES
with open(os.path.join(GOLDEN_DIR, "train_golden_meta.json")) as _f:
    REFERENCE_DEVIATION = json.load(_f)["gpu_cases"]     # the reference's own fp32 deviation from its fp64 run, per case
DEV = torch.device("cuda")
_cache = {}


def case(name):
    """The case's inputs and its fp64 oracle, computed once and shared (read-only) by the tests."""
    if name not in _cache:
        inputs, focal = CASES[name]
        x, y, pairs, target = train_oracle.make_head_case(**inputs)
        cls = train_oracle.classes(target)
        _cache[name] = dict(x=x, y=y, pairs=pairs, target=target, cls=cls, focal=focal, inputs=inputs, oracle=train_oracle.head(x, y, cls, **focal))
    return _cache[name]


def gpu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(DEV) if dtype is None else t.to(DEV, dtype)


def workspace(b, n, m, fill=None):
    nbytes = _native_train.load().gtr_workspace_bytes(b, n, m)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    if fill is not None:
        ws.fill_(fill)
    return ws


def run_head(c, grads=True, fill=None):
    x, y, cls = gpu(c["x"]), gpu(c["y"]), gpu(c["cls"])
    b, _, n = x.shape
    m = y.shape[2]
    f = c["focal"]
    ws = workspace(b, n, m, fill)
    loss, counts = torch.full((1,), float("nan"), device=DEV), torch.full((3,), -1, dtype=torch.int64, device=DEV)
    dx, dy = (torch.full_like(x, float("nan")), torch.full_like(y, float("nan"))) if grads else (None, None)
    _native_train.call("gtr_loss_head", DEV, x, y, cls, b, n, m, f["alpha"], f["gamma"], f["pos_w"], f["neg_w"], f["scale"], loss, counts,
                       dx, dy, ws, ws.numel())
    torch.cuda.synchronize()
    return loss, counts, dx, dy


def rel_err(got, want):
    """max|d| / max|want|; 0 / 0 (an all-zero oracle met exactly) is 0"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    top, d = np.abs(want).max(), np.abs(got - want).max()
    return 0.0 if d == 0.0 else d / top if top > 0 else float("inf")


def bounds(name):
    """(loss bound, gradient bound) of a case: the floors, or 4 x the reference's own recorded deviation where that is larger"""
    dev = REFERENCE_DEVIATION.get(name) or dict(loss=0.0, dx=0.0, dy=0.0)       # "neither": the reference asserts, nothing recorded
    return max(LOSS_RTOL, 4 * dev["loss"]), max(GRAD_RTOL, 4 * max(dev["dx"], dev["dy"]))


def check_loss(got, want, what, bound=LOSS_RTOL):
    err = 0.0 if got == want else abs(got - want) / abs(want) if want != 0 else float("inf")
    print(f"{what}: loss {got!r} oracle {want!r} relative error {err:.3e} (bound {bound:.1e})")
    assert err <= bound, what


def check_grad(got, want, what, bound=GRAD_RTOL):
    err = rel_err(got.cpu().numpy() if isinstance(got, torch.Tensor) else got, want)
    print(f"{what}: max|d| / max|oracle| = {err:.3e} (max|oracle| {np.abs(want).max():.3e}, bound {bound:.1e})")
    assert err <= bound, what


@pytest.mark.parametrize("name", sorted(CASES))
def test_whole_head_against_the_fp64_oracle(name):
    c = case(name)
    o = c["oracle"]
    loss, counts, dx, dy = run_head(c)
    assert counts.tolist() == o["counts"].tolist()
    lb, gb = bounds(name)
    check_loss(float(loss.item()), o["loss"], name, lb)
    check_grad(dx, o["dx"], name + " dx", gb)
    check_grad(dy, o["dy"], name + " dy", gb)
    if "neither" in name:
        assert loss.item() == 0.0 and not dx.any() and not dy.any() and counts.tolist() == [0, 0, 1]
    # forward only: the same loss bits, no gradient buffers
    loss_f, counts_f, _, _ = run_head(c, grads=False)
    assert torch.equal(loss_f, loss) and torch.equal(counts_f, counts)


@pytest.mark.parametrize("name", ["1x1x1_only_positive", "2x129x65_pad0_gamma1.5", "2x200x333", "3x128x64_ignored_band"])
def test_two_calls_and_a_dirty_workspace_give_the_same_bits(name):
    c = case(name)
    first = run_head(c, fill=0)
    again = run_head(c)
    dirty = run_head(c, fill=0xFF)                       # every float of the workspace a NaN, every int -1
    for a, b, d in zip(first, again, dirty):
        assert torch.equal(a, b) and torch.equal(a, d)
        assert not torch.isnan(a.float()).any()


@pytest.mark.parametrize("name", sorted(CASES))
def test_stage_scores_exp(name):
    c = case(name)
    o = c["oracle"]
    x, y = gpu(c["x"]), gpu(c["y"])
    b, _, n = x.shape
    m = y.shape[2]
    E, r, cc = (torch.full(s, float("nan"), device=DEV) for s in ((b, n, m), (b, n), (b, m)))
    ws = workspace(b, n, m, 0xFF)
    _native_train.call("gtr_scores_exp", DEV, x, y, b, n, m, c["focal"]["scale"], E, r, cc, ws, ws.numel())
    for got, want, what in ((E, o["E"], "E"), (r, o["r"], "r"), (cc, o["c"], "c")):
        err = np.abs(got.cpu().numpy().astype(np.float64) / want - 1).max()
        print(f"{name} {what}: max relative error {err:.3e}")
        assert err <= E_RTOL, what


def stage_inputs(c):
    """E, r, c of the oracle rounded to fp32: what the later stages are given, and what the oracle is evaluated at"""
    o = c["oracle"]
    return o["E"].astype(np.float32), o["r"].astype(np.float32), o["c"].astype(np.float32)


@pytest.mark.parametrize("name", sorted(CASES))
def test_stage_loss_terms(name):
    c = case(name)
    f = c["focal"]
    E, r, cc = stage_inputs(c)
    kw = {k: f[k] for k in ("alpha", "gamma", "pos_w", "neg_w")}
    o = train_oracle.loss_terms(E, r, cc, c["cls"], **kw)
    b, n, m = E.shape
    sums, counts, loss = torch.empty(2, dtype=torch.float64, device=DEV), torch.empty(3, dtype=torch.int64, device=DEV), torch.empty(1, device=DEV)
    rowh, colh = torch.full((b, n), float("nan"), device=DEV), torch.full((b, m), float("nan"), device=DEV)
    ws = workspace(b, n, m, 0xFF)
    _native_train.call("gtr_loss_terms", DEV, gpu(E), gpu(r), gpu(cc), gpu(c["cls"]), b, n, m, f["alpha"], f["gamma"], f["pos_w"], f["neg_w"],
                       sums, counts, loss, rowh, colh, ws, ws.numel())
    assert counts.tolist() == o["counts"].tolist()
    lb, gb = bounds(name)
    check_loss(float(loss.item()), o["loss"], name, lb)
    for i, what in enumerate(("sum over the positives", "sum over the negatives")):
        check_loss(float(sums[i].item()), float(o["loss_sums"][i]), f"{name} {what}", lb)
    check_grad(rowh, o["rowsum_h"], name + " rowsum(H)", gb)
    check_grad(colh, o["colsum_h"], name + " colsum(H)", gb)


@pytest.mark.parametrize("name", sorted(CASES))
def test_stage_score_grad(name):
    c = case(name)
    f = c["focal"]
    E, r, cc = stage_inputs(c)
    kw = {k: f[k] for k in ("alpha", "gamma", "pos_w", "neg_w")}
    t = train_oracle.loss_terms(E, r, cc, c["cls"], **kw)
    rowh, colh = t["rowsum_h"].astype(np.float32), t["colsum_h"].astype(np.float32)
    want = train_oracle.score_grad(E, r, cc, c["cls"], t["counts"], rowh, colh, **kw)
    b, n, m = E.shape
    dS = torch.full((b, n, m), float("nan"), device=DEV)
    ws = workspace(b, n, m, 0xFF)
    _native_train.call("gtr_score_grad", DEV, gpu(E), gpu(r), gpu(cc), gpu(c["cls"]), gpu(t["counts"]), gpu(rowh), gpu(colh), b, n, m,
                       f["alpha"], f["gamma"], f["pos_w"], f["neg_w"], dS, ws, ws.numel())
    check_grad(dS, want, name + " dS", bounds(name)[1])


def test_build_target_equals_reshape_assign_matrix():
    with open(os.path.join(GOLDEN_DIR, "train_golden_meta.json")) as fh:
        meta = json.load(fh)["assign"]
    g = load_golden("train_assign")
    for name, s in meta.items():
        pairs = torch.from_numpy(g[name + ".pairs"])
        with_negative = torch.cat([pairs, torch.tensor([[-1, 2, -3], [0, -5, -1]], dtype=pairs.dtype)], dim=1)
        target = SparseTarget([pairs, with_negative, pairs[:, :0]], [s["n_orig"]] * 3, [s["m_orig"]] * 3, pad_val=s["pad_val"])
        cls = target.classes(s["n"], s["m"], DEV).cpu().numpy()
        want = train_oracle.classes(g[name + ".target"])
        np.testing.assert_array_equal(cls[0], want)
        np.testing.assert_array_equal(cls[1], want)                     # a negative index is ignored ...
        assert target.negative_pairs.item() == 3                       # ... and counted
        np.testing.assert_array_equal(cls[2], train_oracle.classes(train_oracle.reshape_assign(np.zeros((2, 0)), s["n_orig"], s["m_orig"], s["n"], s["m"], s["pad_val"])))


def module_loss(c, impl, target=None, dtype=torch.float32):
    f = c["focal"]
    crit = MatchingLoss(alpha=f["alpha"], gamma=f["gamma"], pos_weights=f["pos_w"], neg_weights=f["neg_w"], scale_factor=f["scale"], impl=impl)
    x, y = gpu(c["x"], dtype).requires_grad_(), gpu(c["y"], dtype).requires_grad_()
    loss = crit(x, y, gpu(c["target"]) if target is None else target)
    (3 * loss).backward()                                               # a grad_output that is not 1
    return loss.detach(), x.grad / 3, y.grad / 3, crit


def test_module_takes_sparse_and_dense_targets_alike():
    c = case("3x128x64_ignored_band")
    i = c["inputs"]
    dense = module_loss(c, "hip")
    sparse = module_loss(c, "hip", SparseTarget([torch.from_numpy(p) for p in c["pairs"]], i["n_orig"], i["m_orig"], pad_val=i["pad_val"]))
    assert torch.equal(dense[0], sparse[0]) and torch.equal(dense[1], sparse[1]) and torch.equal(dense[2], sparse[2])
    assert dense[3].last_counts.tolist() == c["oracle"]["counts"].tolist() == sparse[3].last_counts.tolist()
    check_loss(float(dense[0].item()), c["oracle"]["loss"], "module")
    check_grad(dense[1], c["oracle"]["dx"], "module dx (grad_output 3)")
    with torch.no_grad():                                               # no autograd: forward only
        crit = MatchingLoss(impl="hip")
        assert torch.equal(crit(gpu(c["x"]), gpu(c["y"]), gpu(c["target"])), dense[0])


def test_hip_head_against_eager_at_2x1000x2000():
    """Both against the eager head in fp64 on the same GPU (the reference's arithmetic, widened): hip within the bounds above (the reference's
    own deviation on this case is recorded with the others); eager's fp32 deviation here is printed, and hip - eager is within the sum."""
    x, y, pairs, target = train_oracle.make_head_case(**train_oracle.BIG_CASE)
    c = dict(x=x, y=y, target=target, focal=DEFAULT)
    lb, gb = bounds(train_oracle.BIG_CASE_NAME)
    ref = module_loss(c, "eager", dtype=torch.float64)
    hip, eager = module_loss(c, "hip"), module_loss(c, "eager")
    assert hip[3].last_counts.tolist() == eager[3].last_counts.tolist() == [600, 2 * 1000 * 2000 - 600, 0]
    want = float(ref[0].item())
    assert 0.5 < want < 5.0                                        # the recipe at work: neither saturated nor untrained-flat
    check_loss(float(hip[0].item()), want, "hip", lb)
    e_loss = abs(float(eager[0].item()) - want) / want
    print(f"eager fp32 loss relative deviation {e_loss:.3e}")
    assert abs(float(hip[0].item()) - float(eager[0].item())) <= (lb + e_loss) * want
    for i, what in ((1, "dx"), (2, "dy")):
        r = ref[i].cpu().numpy()
        check_grad(hip[i], r, "hip " + what, gb)
        e = rel_err(eager[i].cpu().numpy(), r)
        print(f"eager fp32 {what}: max|d| / max|fp64| = {e:.3e}")
        assert rel_err(hip[i].cpu().numpy(), eager[i].cpu().numpy().astype(np.float64)) <= (gb + e) * 1.001


@pytest.fixture(scope="module")
def network():
    with open(os.path.join(GOLDEN_DIR, "train_golden_meta.json")) as fh:
        meta = json.load(fh)["network"]
    inputs = dict(meta["inputs"], noise=tuple(meta["inputs"]["noise"]))
    assert (inputs["num_leaf"], inputs["n1"], inputs["n2"]) == (8, 64, 96)
    data = {k: torch.from_numpy(v).to(DEV) for k, v in synthetic.make_inputs(**inputs).items()}
    return meta, data, torch.from_numpy(load_golden("train_network")["target"]).to(DEV)


def test_one_training_step_parameter_gradients_hip_against_eager(network):
    """num_leaf = 8, 64 x 96: the same trunk, the two heads.  Per tensor the bound is the one the CPU test holds impl="eager" to against
    the reference (max(2e-6, 4 x the reference's recorded fp32 deviation of that tensor)): dx, dy of the two heads differ by fp32 rounding,
    and the trunk's backward amplifies that as it amplifies its own."""
    meta, data, target = network
    grads = {}
    for impl in ("hip", "eager"):
        model = onepose_amd.GATsSuperGlue(dict(meta["hparams"])).to(DEV)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.make_state_dict(meta["weights"][1]).items()}, strict=True)
        loss = training_loss(model, data, target, MatchingLoss(impl=impl, scale_factor=meta["hparams"]["scale_factor"]))
        loss.backward()
        grads[impl] = (loss.item(), {k: p.grad.cpu().numpy().astype(np.float64) for k, p in model.named_parameters() if p.grad is not None})
    (l_hip, g_hip), (l_eager, g_eager) = grads["hip"], grads["eager"]
    assert abs(l_hip - l_eager) <= 2 * LOSS_RTOL * abs(l_eager) and abs(l_hip - meta["loss"]) <= 1e-5 * meta["loss"]
    assert set(g_hip) == set(g_eager) == set(meta["fp32_deviation"]["grads"])
    worst = 0.0
    for k, d in meta["fp32_deviation"]["grads"].items():
        if d["zero"]:
            assert np.abs(g_hip[k]).max() <= 4 * d["fp32_absmax"] + 1e-30, k
            continue
        err = rel_err(g_hip[k], g_eager[k])
        worst = max(worst, err / max(GRAD_RTOL, 4 * d["deviation"]))
        assert err <= max(GRAD_RTOL, 4 * d["deviation"]), (k, err)
    print(f"largest error as a fraction of its bound: {worst:.3f}")


def test_hip_forward_sees_the_weights_after_adam_steps():
    """A few Adam steps (reference hyper-parameters) on planted frames from the trained weights; then the module's HIP forward equals
    the oracle forward on the updated state_dict within the forward's 1e-4 -- the packed blob was re-validated -- and differs from
    the forward before the steps by far more."""
    from oracle import torch_oracle
    hp = dict(descriptor_dim=256, keypoints_encoder=[32, 64, 128], match_type="softmax", scale_factor=0.07, match_threshold=0.2,
              include_self=True, additional=False, with_linear_transform=False)
    model = onepose_amd.GATsSuperGlue(hp).to(DEV)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.make_trained_state_dict().items()}, strict=True)
    shape = dict(b=2, n1=64, n2=96, num_leaf=8, planted=True, noise=(0.3, 0.5))
    probe = {k: torch.from_numpy(v).to(DEV) for k, v in synthetic.make_inputs(seed=77, **shape).items()}
    with torch.no_grad():
        before = model.forward_batched(probe)[0].clone()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=0.0)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[30, 60, 90], gamma=0.5)
    crit = MatchingLoss(impl="hip")
    losses = []
    for step in range(3):
        d, tg = synthetic.make_inputs(seed=500 + step, with_targets=True, **shape)
        data = {k: torch.from_numpy(v).to(DEV) for k, v in d.items()}
        pairs = [torch.stack([torch.arange(tg.shape[1]), torch.from_numpy(tg[bi]).long()]) for bi in range(shape["b"])]
        loss = training_loss(model, data, SparseTarget(pairs, shape["n1"], shape["n2"]), crit)
        opt.zero_grad()
        loss.backward()
        opt.step()
        sched.step()
        losses.append(loss.item())
    assert all(np.isfinite(losses)) and crit.last_counts[0].item() == shape["b"] * tg.shape[1]
    with torch.no_grad():
        after = model.forward_batched(probe)[0]
        _, want = torch_oracle.forward({k: v.detach() for k, v in model.state_dict().items()}, probe, hp)
    moved = (after - before).abs().max().item()
    err = (after - want).abs().max().item()
    print(f"losses {losses}; conf moved by {moved:.3e}; HIP forward - oracle forward on the new weights {err:.3e}")
    assert err <= 1e-4 and moved > 10 * 1e-4
