"""GPU: the derived copies of the weights stay coherent with the f32 weights over any sequence of operations, not only on a fresh model.

runtime.FlatParams keeps, next to the flat f32 parameters, a bf16 shadow (w16), an fp16 shadow (wh16) and - once the hybrid mode has used
it - the fp16 lo shadow wl16 = fp16(w - fp16(w)): a hybrid-mode product contracts hi and lo, so a zero or stale lo quietly turns it into a
plain fp16 product (fp16 accuracy instead of the hybrid mode's).  The engine derives more copies from them (re-laid-out taps and patch
matrices, the fused feed-forward hi / lo packs, positional projections).

* the flat shadows, bit for bit, after every optimizer step (eager in each mode, captured in fp16 / hybrid), a skipped step, a
  load_state_dict, an in-place torch edit and every switch into the hybrid mode after training in another mode;
* a model trained in mode A (eagerly or captured) and switched to mode B computes, bit for bit, what a freshly built model carrying the
  same state_dict computes in B - for all sixteen (A, B) pairs - so every derived-weight cache followed the switch."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T, B = 16, 4
MODES = ["fp32", "bf16", "fp16", "hybrid"]


def _set_dropout(m, p):
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = p


def _make(seed=5, sd=None):
    from sar_ssl_amd import model, runtime
    dev = torch.device("cuda:0")
    torch.manual_seed(seed)
    net = model.SARSSL(sig_shape=(256, T, 2, 2), pretrain=True, device=dev)
    if sd is not None:
        net.load_state_dict(sd)
    _set_dropout(net, 0.0)
    net.to(dev).train()
    return net, runtime.FlatParams(net)


def _batches(n, seed=3):
    from sar_ssl_amd import hip, synth
    sig = torch.from_numpy(synth.make_batch(seed, n * B, nsample=512 + 256 * (T - 1))).cuda()
    return [hip.stft_frontend(sig[i * B:(i + 1) * B]) for i in range(n)]


def _masks(net):
    random.seed(2024)
    idx, ch = net.patch_mask.sample(B, 2)
    return np.asarray(idx), np.asarray(ch)


def _eval(net, x, masks):
    """One eval forward in the current mode: (loss, diff, pred) copies."""
    net.eval()
    try:
        with torch.no_grad():
            net.set_masks(*masks)
            loss, diff, vis = net(x)
            out = (loss.detach().float().clone(), diff.detach().float().clone(), vis["pred"].detach().float().clone())
    finally:
        net.train()
    torch.cuda.synchronize()
    return out


def _coherent(flat, where):
    torch.cuda.synchronize()
    f = flat.flat
    assert torch.equal(flat.w16, f.bfloat16()), "%s: bf16 shadow != bf16(flat)" % where
    assert torch.equal(flat.wh16, f.half()), "%s: fp16 shadow != fp16(flat)" % where
    if flat.wl16 is not None:
        want = (f - f.half().float()).half()
        bad = int((flat.wl16 != want).sum())
        assert bad == 0, "%s: lo shadow != fp16(flat - fp16(flat)) at %d of %d entries" % (where, bad, f.numel())


def _train(net, flat, xs, form, opt=None):
    """len(xs) training steps in the current mode: launch by launch through runtime.FusedAdam, or captured (graph.PretrainStepGraph).
    ``opt``: the optimizer / captured step of earlier calls (reused while the mode is the same)."""
    from sar_ssl_amd import runtime
    from sar_ssl_amd.graph import PretrainStepGraph
    if form == "eager":
        opt = opt or runtime.FusedAdam(flat, lr=1e-3)
        for x in xs:
            opt.zero_grad()
            loss, _, _ = net(x)
            loss.backward()
            opt.step(guard=loss.detach())
    else:
        opt = opt or PretrainStepGraph(net, flat, lr=1e-3)
        for x in xs:
            opt.step(x=x)
    torch.cuda.synchronize()
    return opt


def test_flat_shadows_stay_coherent_over_transitions():
    from sar_ssl_amd import runtime
    try:
        xs = _batches(3)
        net, flat = _make()
        masks = _masks(net)
        random.seed(11)
        _coherent(flat, "fresh")
        for mode in ("fp32", "bf16", "fp16", "hybrid"):
            runtime.set_precision(mode)
            if mode == "hybrid":
                _eval(net, xs[0], masks)                       # first hybrid use: allocates the lo shadow
                _coherent(flat, "fp16 step -> hybrid eval")
            _train(net, flat, xs[:1], "eager")
            _coherent(flat, "FusedAdam step in %s" % mode)
        for mode in ("fp16", "hybrid"):
            runtime.set_precision(mode)
            _train(net, flat, xs[:2], "captured")
            _coherent(flat, "two captured steps in %s" % mode)
        _eval(net, xs[0], masks)
        _coherent(flat, "hybrid eval after the captured steps")
        # a step whose guard is not finite: nothing moves, the shadows stay what they were
        before = (flat.flat.clone(), flat.wh16.clone(), flat.wl16.clone())
        opt = runtime.FusedAdam(flat, lr=1e-3)
        opt.zero_grad()
        loss, _, _ = net(xs[1])
        loss.backward()
        opt.step(guard=torch.full((1,), float("nan"), device=flat.flat.device))
        _coherent(flat, "skipped step")
        assert int(opt.nskipped.item()) == 1
        assert all(torch.equal(a, b) for a, b in zip(before, (flat.flat, flat.wh16, flat.wl16)))
        # through torch: the shadows follow at the next forward (begin_forward -> ensure_shadow)
        net2, _ = _make(seed=6)
        net.load_state_dict(net2.state_dict())
        _eval(net, xs[0], masks)
        _coherent(flat, "load_state_dict")
        with torch.no_grad():
            for p in net.parameters():
                p.mul_(1.25)
        _eval(net, xs[0], masks)
        _coherent(flat, "in-place torch edit")
        runtime.set_precision("fp16")
        _train(net, flat, xs[:1], "eager")
        _coherent(flat, "FusedAdam step in fp16 with the lo shadow allocated")
    finally:
        runtime.set_precision("bf16")


@pytest.mark.parametrize("form", ["eager", "captured"])
@pytest.mark.parametrize("mode_a", ["fp32", "bf16", "fp16"])
def test_switch_into_hybrid_after_training_in_another_mode(mode_a, form):
    """Train in mode_a -> hybrid eval -> train in mode_a again -> hybrid eval: the lo shadow the hybrid forward reads must be that of the
    current weights both times (round-6 advisor finding: the first switch used an all-zero lo shadow; the captured step of a mode without
    the lo shadow left it stale at the second)."""
    from sar_ssl_amd import runtime
    try:
        xs = _batches(4)
        net, flat = _make()
        masks = _masks(net)
        random.seed(11)
        runtime.set_precision(mode_a)
        opt = _train(net, flat, xs[:2], form)
        runtime.set_precision("hybrid")
        _eval(net, xs[0], masks)
        _coherent(flat, "%s %s steps -> hybrid" % (mode_a, form))
        runtime.set_precision(mode_a)
        _train(net, flat, xs[2:], form, opt)
        _coherent(flat, "%s %s steps after a hybrid eval" % (mode_a, form))
        runtime.set_precision("hybrid")
        _eval(net, xs[0], masks)
        _coherent(flat, "%s %s steps -> hybrid, twice" % (mode_a, form))
    finally:
        runtime.set_precision("bf16")


@pytest.mark.parametrize("form", ["eager", "captured"])
@pytest.mark.parametrize("mode_b", MODES)
@pytest.mark.parametrize("mode_a", MODES)
def test_switched_model_equals_fresh_model(mode_a, mode_b, form):
    """Three training steps in mode_a, set_precision(mode_b), eval forward == a fresh model loaded with the same state_dict, in mode_b, bit
    for bit (loss, diff and the prediction at every frame).  The fresh model is run twice first: the eval forward is bit-reproducible
    run to run in every mode (the statistics' f64 atomics are rounded back to f32 once, the folds are ordered)."""
    from sar_ssl_amd import runtime
    try:
        xs = _batches(3)
        net, flat = _make()
        masks = _masks(net)
        random.seed(11)
        runtime.set_precision(mode_a)
        _train(net, flat, xs, form)
        runtime.set_precision(mode_b)
        got = _eval(net, xs[0], masks)
        _coherent(flat, "%s -> %s" % (mode_a, mode_b))
        sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
        fresh, _ = _make(seed=99, sd=sd)
        want = _eval(fresh, xs[0], masks)
        again = _eval(fresh, xs[0], masks)
        for name, a, b in zip(("loss", "diff", "pred"), want, again):
            assert torch.equal(a, b), "fresh model in %s is not run-to-run reproducible (%s)" % (mode_b, name)
        for name, a, b in zip(("loss", "diff", "pred"), got, want):
            d = float((a - b).abs().max())
            assert torch.equal(a, b), "%s -> %s (%s): %s differs from a fresh model by %.3e" % (mode_a, mode_b, form, name, d)
    finally:
        runtime.set_precision("bf16")
