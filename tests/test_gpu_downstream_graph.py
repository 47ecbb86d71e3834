"""GPU: the captured downstream steps (sar_ssl_amd/graph.py, DownstreamStepGraph) - against their launch-by-launch twins, against the
reference's fine-tuning trajectory (fixture F9, as tests/test_gpu_downstream.py), and through the learner's train_epoch / test_epoch."""
import numpy as np
import pytest
import torch

from conftest import check
from test_gpu_downstream import TOL, _set_dropout, _setup

pytestmark = pytest.mark.gpu


def _make(T, mode, embed="spat", p_drop=None, seed=11):
    """A downstream model with seeded weights (dropout at its default unless p_drop is given) and its flat buffers."""
    from sar_ssl_amd import model, runtime
    dev = torch.device("cuda:0")
    torch.manual_seed(seed)
    net = model.SARSSL(sig_shape=(256, T, 2, 2), pretrain=False, device=dev, downstream_token="all", downstream_head="mlp",
                       downstream_embed=embed, downstream_dlabel=1)
    if p_drop is not None:
        _set_dropout(net, p_drop)
    if mode == "lineareval":
        for k, v in net.named_parameters():
            if k.startswith(("spec_encoder.", "spat_encoder.")):
                v.requires_grad = False
    net.to(dev).train()
    return net, runtime.FlatParams(net)


def _batches(T, n, B, seed=3):
    """n raw batches (B, nsample, 2) f32 on the GPU and their targets (B, 1), a few samples of delay."""
    from sar_ssl_amd import synth
    nsample = 512 + 256 * (T - 1)
    sig = torch.from_numpy(synth.make_batch(seed, n * B, nsample=nsample)).cuda()
    tar = torch.from_numpy(np.random.default_rng(seed).uniform(-8.0, 8.0, (n * B, 1)).astype(np.float32)).cuda()
    return [(sig[i * B:(i + 1) * B].contiguous(), tar[i * B:(i + 1) * B].contiguous()) for i in range(n)]


def _run_twin(form, prec, mode, embed, T=16, B=4, n=4, lr=1e-3):
    from sar_ssl_amd.graph import DownstreamStepGraph
    net, flat = _make(T, mode, embed)
    p0 = flat.flat.clone()
    g = DownstreamStepGraph(net, flat, lr=lr)
    outs = []
    for sig, tar in _batches(T, n, B):
        outs.append((g.step if form == "captured" else g.step_eager)(pcm=sig, target=tar).clone())
    torch.cuda.synchronize()
    if form == "captured":
        assert len(g._plans[True][0]) == 1                                    # one graph per step
    return torch.stack(outs).cpu(), flat.flat.clone(), [(k, b.clone()) for k, b in net.named_buffers()], p0, g


def _twin_case(mode, embed, prec):
    from sar_ssl_amd import runtime
    runtime.set_precision(prec)
    try:
        lr = 1e-3
        out_a, flat_a, bufs_a, p0, g = _run_twin("captured", prec, mode, embed, lr=lr)
        out_b, flat_b, bufs_b, _, _ = _run_twin("eager", prec, mode, embed, lr=lr)
        assert torch.isfinite(out_a).all() and g.skipped_steps() == 0
        assert float((flat_a - p0).abs().max()) > 0                           # the steps did train
        if prec != "fp32":
            assert torch.equal(out_a, out_b), (out_a, out_b)
            assert torch.equal(flat_a, flat_b)
            for (k, a), (_, b) in zip(bufs_a, bufs_b):
                assert torch.equal(a, b), k
        else:
            check("ds_graph_vs_eager.%s.loss" % mode, float(((out_a - out_b).abs() / out_b.abs()).max()), 2e-5)
            check("ds_graph_vs_eager.%s.frac_params_off_by_half_lr" % mode, float((flat_a - flat_b).abs().gt(0.5 * lr).float().mean()), 1e-3)
            check("ds_graph_vs_eager.%s.param_diff_norm_over_update_norm" % mode, float((flat_a - flat_b).norm() / (flat_b - p0).norm()), 2e-2)
            for (k, a), (_, b) in zip(bufs_a, bufs_b):
                if k.endswith("num_batches_tracked"):
                    assert int(a) == int(b) == 4, k                           # the capture warm-up left no trace
                elif "running" in k:
                    assert float((a - b).abs().max()) <= 1e-4 * float(a.abs().max()) + 1e-6, k
    finally:
        runtime.set_precision("bf16")


@pytest.mark.parametrize("prec", ["fp16", "hybrid", "bf16", "fp32"])
@pytest.mark.parametrize("mode", ["finetune", "lineareval"])
def test_captured_step_equals_its_eager_twin(mode, prec):
    """T = 16, B = 4, 4 steps, dropout at its default 0.1: the replayed step and the same body enqueued launch by launch (same device
    salt, same static seeds).  16-bit modes: parameters, BatchNorm buffers and the per-step loss words bit for bit; fp32 (not run-to-run
    exact) under the gates of test_gpu_graph.test_graph_step_equals_eager_step."""
    _twin_case(mode, "spat", prec)


def test_captured_step_equals_its_eager_twin_spec_spat():
    """The head on both encoders' embeddings (downstream_embed='spec_spat'), in the mode --use-amp selects."""
    _twin_case("finetune", "spec_spat", "hybrid")


@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16", "hybrid"])
@pytest.mark.parametrize("mode", ["finetune", "lineareval"])
def test_captured_steps_vs_reference(mode, prec):
    """F9 (B = 4, T = 64, dropout 0): three replayed steps against the reference's per-step loss, metric and predictions, under the
    tolerance rows of tests/test_gpu_downstream.py."""
    from sar_ssl_amd import runtime
    from sar_ssl_amd.graph import DownstreamStepGraph
    tol = TOL[prec]
    try:
        z, ds, lrn, loader = _setup(mode, prec)
        ds.train()
        g = DownstreamStepGraph(ds, lrn._flat, lr=float(z["lr"]))
        assert (len(g.frozen) > 0) == (mode == "lineareval")
        worst = dict(loss=0.0, pred=0.0)
        for s, (sig, gt) in enumerate(loader):
            tar = lrn.get_tar_batch(gt["TDOA"].cuda())
            out = g.step(pcm=sig.cuda(), target=tar)
            loss, metric = [float(v) for v in out]
            lref, mref = float(z[mode + ".loss"][s]), float(z[mode + ".metric"][s])
            worst["loss"] = max(worst["loss"], abs(loss - lref) / lref, abs(metric - mref) / mref)
            p_ref = torch.from_numpy(z[mode + ".pred"][s]).to(g.pred.device)
            worst["pred"] = max(worst["pred"], float((g.pred - p_ref).abs().max() / p_ref.abs().max()))
        assert g.nsteps == 3 and len(g._plans[True][0]) == 1
        for k in ("loss", "pred"):
            check("tdoa_graph.%s.%s.%s" % (mode, prec, k), worst[k], tol[k])
    finally:
        runtime.set_precision("bf16")


@pytest.mark.parametrize("mode", ["finetune", "lineareval"])
def test_learner_epochs_through_the_graph_vs_reference(mode):
    from sar_ssl_amd import runtime
    from sar_ssl_amd.graph import DownstreamStepGraph
    tol = TOL["fp32"]
    try:
        z, ds, lrn, loader = _setup(mode, "fp32")
        ltr, mtr = lrn.train_epoch(loader, lr=float(z["lr"]), epoch=1, return_metric=True)
        lte, mte, vis = lrn.test_epoch(loader, return_metric=True, return_vis=True)
        g = lrn.__dict__.get("_step_graph")
        assert isinstance(g, DownstreamStepGraph) and sorted(g._plans) == [False, True]      # the learner did build and replay both variants
        ref_tr, ref_te = z[mode + ".train_epoch"], z[mode + ".test_epoch"]
        assert abs(ltr - ref_tr[0]) <= tol["epoch"] * ref_tr[0] and abs(float(mtr) - ref_tr[1]) <= tol["epoch"] * ref_tr[1]
        assert abs(lte - ref_te[0]) <= tol["epoch"] * ref_te[0] and abs(float(mte) - ref_te[1]) <= tol["epoch"] * ref_te[1]
        assert vis["embed"].shape == (12, 256) and vis["label"].shape == (12, 1)
    finally:
        runtime.set_precision("bf16")


def test_lineareval_leaves_the_encoders_alone():
    """Frozen encoders: parameters bit-identical to their initial values after the steps, frozen ranges of the gradient buffer zero
    (the Adam pass's zero_grad is switched off to read it), the head's gradient is not."""
    from sar_ssl_amd import runtime
    from sar_ssl_amd.graph import DownstreamStepGraph
    runtime.set_precision("hybrid")
    try:
        T, B = 16, 4
        net, flat = _make(T, "lineareval")
        init = {k: v.detach().clone() for k, v in net.named_parameters()}
        g = DownstreamStepGraph(net, flat, lr=1e-3)
        g.zero_grad_in_adam = False
        for sig, tar in _batches(T, 3, B):
            g.step(pcm=sig, target=tar)
        torch.cuda.synchronize()
        assert g.frozen
        for s, e in g.frozen:
            assert float(flat.grad[s:e].abs().max()) == 0.0
        assert float(flat.grad.abs().max()) > 0
        moved = 0
        for k, v in net.named_parameters():
            if k.startswith(("spec_encoder.", "spat_encoder.")):
                assert torch.equal(v.detach(), init[k]), k
            else:
                moved += int(not torch.equal(v.detach(), init[k]))
        assert moved > 0
    finally:
        runtime.set_precision("bf16")


def test_inputs_reach_the_replay_and_the_host_is_out_of_the_step():
    """lr = 0 and dropout off: every replay computes the same function of (PCM, target).  And one replayed step costs the host at most
    a tenth of the library calls its launch-by-launch twin issues, training and evaluation alike."""
    from sar_ssl_amd import runtime, _lib
    from sar_ssl_amd.graph import DownstreamStepGraph
    runtime.set_precision("hybrid")
    try:
        T, B = 16, 4
        net, flat = _make(T, "finetune", p_drop=0.0)
        g = DownstreamStepGraph(net, flat, lr=0.0)
        (s0, t0), (s1, t1) = _batches(T, 2, B)
        for train in (True, False):
            net.train(train)
            run, twin = (g.step, g.step_eager) if train else (g.eval_step, g.eval_step_eager)
            a = run(pcm=s0, target=t0).clone()
            pa = g.pred.clone()
            n0 = _lib.ncalls
            a2 = run(pcm=s0, target=t0).clone()
            n_replay = _lib.ncalls - n0
            assert torch.equal(a, a2) and torch.equal(pa, g.pred)
            b = run(pcm=s0, target=t1).clone()
            assert torch.equal(pa, g.pred) and float(b[0]) != float(a[0])          # another target: same prediction, another loss
            run(pcm=s1, target=t0)
            assert not torch.equal(pa, g.pred)                                      # another batch: another prediction
            n0 = _lib.ncalls
            c = twin(pcm=s0, target=t0).clone()
            n_eager = _lib.ncalls - n0
            assert torch.equal(c, a) and torch.equal(pa, g.pred)
            print("downstream %s step: %d library calls replayed, %d launch by launch" % ("train" if train else "eval", n_replay, n_eager))
            assert n_eager > 50 and 10 * n_replay <= n_eager, (n_replay, n_eager)
        assert g.acc_eval.cpu().tolist()[2] == 5.0 and g.acc.cpu().tolist()[2] == 5.0
    finally:
        runtime.set_precision("bf16")


@pytest.mark.parametrize("prec", ["fp32", "hybrid"])
def test_eval_replay_follows_the_trained_weights(prec, monkeypatch):
    """test_epoch, one train_epoch, test_epoch again - all replayed.  The second evaluation must see the weights the training replays
    wrote: it equals the launch-by-launch evaluation (SARSSL_GRAPH=0) of the same weights - loss and metric within 5e-4 (the gate of
    test_learner_epoch_graph_equals_eager_incl_ragged_tail_and_epoch_reset); in hybrid the pooled embeddings, which both paths form with
    the same kernels, bit for bit, and the loss words to 1e-6 (the launch-by-launch loss is torch's f32 mean of four squares, the
    replayed one an f64 sum rounded once: a few f32 ulps apart at most)."""
    from sar_ssl_amd import runtime
    from sar_ssl_amd.graph import DownstreamStepGraph
    try:
        monkeypatch.setenv("SARSSL_GRAPH", "1")
        z, ds, lrn, loader = _setup("finetune", prec)
        l0, m0, _ = lrn.test_epoch(loader, return_metric=True, return_vis=True)
        lrn.train_epoch(loader, lr=2e-3, epoch=1)
        l1, m1, v1 = lrn.test_epoch(loader, return_metric=True, return_vis=True)
        g = lrn.__dict__.get("_step_graph")
        assert isinstance(g, DownstreamStepGraph) and sorted(g._plans) == [False, True]
        monkeypatch.setenv("SARSSL_GRAPH", "0")
        l2, m2, v2 = lrn.test_epoch(loader, return_metric=True, return_vis=True)
        gate = 1e-6 if prec == "hybrid" else 5e-4
        assert abs(l1 - l0) > 10 * 5e-4 * abs(l0)                                  # the epoch moved the weights: a stale plan would show
        check("ds_eval_after_train.%s.loss" % prec, abs(l1 - l2) / abs(l2), gate)
        check("ds_eval_after_train.%s.metric" % prec, abs(float(m1) - float(m2)) / abs(float(m2)), gate)
        assert torch.equal(v1["label"], v2["label"])
        if prec == "hybrid":
            assert torch.equal(v1["embed"], v2["embed"].float())
        else:
            check("ds_eval_after_train.fp32.embed", float((v1["embed"] - v2["embed"]).abs().max() / v2["embed"].abs().max()), 5e-4)
    finally:
        runtime.set_precision("bf16")


def test_learner_graph_equals_eager_incl_ragged_tail_and_epoch_reset(monkeypatch):
    """Batches of 4 + 4 + 3 (the last one takes the eager twin), two epochs at two learning rates (Adam restarts per epoch), fp32,
    dropout off: the replayed epochs against SARSSL_GRAPH=0."""
    from sar_ssl_amd import learner as L, model, runtime, synth
    dev = torch.device("cuda:0")
    T = 16
    nsample = 512 + 256 * (T - 1)
    data = torch.from_numpy(synth.make_batch(0, 11, nsample=nsample))
    tdoa = torch.from_numpy(np.random.default_rng(1).uniform(-5e-4, 5e-4, 11).astype(np.float32))
    loader = [(data[a:b], {"TDOA": tdoa[a:b]}) for a, b in ((0, 4), (4, 8), (8, 11))]
    res = {}
    try:
        for mode in ("0", "1"):
            monkeypatch.setenv("SARSSL_GRAPH", mode)
            torch.manual_seed(3)
            net = model.SARSSL(sig_shape=(256, T, 2, 2), pretrain=False, device=dev, downstream_token="all", downstream_head="mlp",
                               downstream_embed="spat", downstream_dlabel=1)
            _set_dropout(net, 0.0)
            lrn = L.STFTLearner(net, win_len=512, win_shift_ratio=0.5, nfft=512, fre_used_ratio=1, fs=16000, task="TDOA", ch_mode="M")
            lrn.cuda()                                                       # fp32 mode
            l1, m1 = lrn.train_epoch(loader, lr=1e-3, epoch=1, return_metric=True)
            l2, m2 = lrn.train_epoch(loader, lr=5e-4, epoch=2, return_metric=True)
            lv, mv, vis = lrn.test_epoch(loader, return_metric=True, return_vis=True)
            res[mode] = (l1, float(m1), l2, float(m2), lv, float(mv), vis)
            if mode == "1":
                g = lrn._step_graph
                assert sorted(g._plans) == [False, True] and g.nsteps == 3 and g._plans[True][1][0] == (4, nsample, 2)
            else:
                assert "_step_graph" not in lrn.__dict__
        a, b = res["0"], res["1"]
        for name, i in (("loss_ep1", 0), ("metric_ep1", 1), ("loss_ep2", 2), ("metric_ep2", 3), ("val_loss", 4), ("val_metric", 5)):
            check("ds_learner_graph_vs_eager." + name, abs(a[i] - b[i]) / abs(a[i]), 5e-4)
        va, vb = a[6], b[6]
        assert vb["embed"].shape == (11, 256) and vb["label"].shape == (11, 1)
        assert torch.equal(va["label"].float(), vb["label"].float())
        check("ds_learner_graph_vs_eager.embed", float((va["embed"].float() - vb["embed"]).abs().max() / va["embed"].abs().max()), 5e-4)
    finally:
        runtime.set_precision("bf16")


def test_a_subclass_loss_is_honoured(monkeypatch):
    """A learner whose class overrides ``loss`` never builds the graph, and its loss is the one that trains."""
    from sar_ssl_amd import learner as L, runtime
    monkeypatch.setenv("SARSSL_GRAPH", "1")

    class Tripled(L.STFTLearner):
        ncalls = 0

        def loss(self, pred_batch, gt_batch):
            self.ncalls += 1
            return 3.0 * super().loss(pred_batch, gt_batch)
    try:
        z, ds, lrn, loader = _setup("finetune", "fp32")
        w0 = lrn._flat.flat.clone()
        plain = lrn.train_epoch(loader[:1], lr=1e-4, epoch=1)
        assert "_step_graph" in lrn.__dict__
        step_plain = lrn._flat.flat - w0
        z, ds, lrn, loader = _setup("finetune", "fp32")
        lrn.__class__ = Tripled
        tripled = lrn.train_epoch(loader[:1], lr=1e-4, epoch=1)
        assert "_step_graph" not in lrn.__dict__ and lrn.ncalls == 1
        check("ds_subclass_loss", abs(tripled - 3.0 * plain) / (3.0 * plain), 1e-5)
        lrn.test_epoch(loader[:1])
        assert "_step_graph" not in lrn.__dict__ and lrn.ncalls == 2
        assert float(step_plain.abs().max()) > 0
    finally:
        runtime.set_precision("bf16")
