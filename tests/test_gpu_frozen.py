"""GPU: the frozen-encoder probe stage (``--pretrain-frozen-encoder``; model._FrozenProbeFn) - the probe-mask launch against its numpy
restatement, one step against the reference (fixture F17) and the learner's epochs against the reference's own (F18) in the four numeric
modes, the guard against trainable encoders, the checkpoint round trip and the command line."""
import importlib.util
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import recipes
from conftest import GOLD, ROOT, check
from test_frozen_cpu import probe_inputs_np

pytestmark = pytest.mark.gpu

MODES = ["fp32", "bf16", "fp16", "hybrid"]
DEC = "spec_spat_decoder."


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _npz(name):
    return np.load(os.path.join(GOLD, name), allow_pickle=False)


def _manifest():
    return json.load(open(os.path.join(GOLD, "state_dict_manifest_frozen.json")))["frozen"]


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_frozen", os.path.join(ROOT, "tools", "make_golden_frozen.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _set_dropout(m, p):
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = p


def _freeze(net):
    """As the command line does (code/run_pretrain.py:364-369): every parameter whose name contains 'encoder'."""
    for k, p in net.named_parameters():
        if "encoder" in k:
            p.requires_grad = False


def _relerr(a, b):
    a = torch.as_tensor(np.asarray(a.detach().float().cpu() if torch.is_tensor(a) else a)).double()
    b = torch.as_tensor(np.asarray(b)).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def _frozen_net(T, dev, weight_seed=0):
    from sar_ssl_amd import model
    net = model.SARSSL(sig_shape=(256, T, 2, 2), pretrain=False, pretrain_frozen_encoder=True, device=dev)
    init = recipes.recipe_state_dict(_manifest(), weight_seed)                    # (the same shapes at every T)
    net.load_state_dict(init)
    _set_dropout(net, 0.0)
    _freeze(net)
    return net, init


def _learner(net):
    from sar_ssl_amd import learner as L
    lrn = L.STFTLearner(net, win_len=512, win_shift_ratio=0.5, nfft=512, fre_used_ratio=1, fs=16000, task=None, ch_mode="M")
    lrn.cuda()
    return lrn


# ---------------------------------------------------------------- 1. the probe-mask launch (sarssl_mask_inputs, mode 2)
def _mask_case(name):
    g = np.random.default_rng(41)
    if name == "b3_f256_t8":                   # more than one block, both masked-channel values
        B, F, T = 3, 256, 8
        idx = [np.sort(g.choice(T, T // 2, replace=False)) for _ in range(B)]
        ch = np.array([1, 0, 1])
    elif name == "b1_f3_t5":                   # nothing divides the block or the vector width
        B, F, T = 1, 3, 5
        idx, ch = [np.array([0, 3])], np.array([0])
    else:                                      # one item with every frame masked, one with none
        B, F, T = 2, 16, 8
        idx, ch = [np.arange(T), np.array([], dtype=np.int64)], np.array([1, 0])
    x = g.standard_normal((B, 2, F, T, 2)).astype(np.float32)
    return x, idx, ch


@pytest.mark.parametrize("case", ["b3_f256_t8", "b1_f3_t5", "all_and_none"])
def test_probe_mask_launch_equals_the_numpy_restatement(case):
    from sar_ssl_amd import hip
    dev = _dev()
    x, idx, ch = _mask_case(case)
    B, _, F, T, _ = x.shape
    mp = np.ones((B, T), dtype=np.uint8)
    for b in range(B):
        mp[b, idx[b]] = 0
    want_spec, want_spat = probe_inputs_np(x, idx, ch)
    xd, mpd, chd = torch.from_numpy(x).to(dev), torch.from_numpy(mp).to(dev), torch.from_numpy(ch.astype(np.int32)).to(dev)
    for dtp in (torch.float32, torch.float16, torch.bfloat16):
        spec, spat = hip.mask_inputs(xd, mpd, chd, 2, dtp)
        assert spec.shape == (B, F, T, 4) and spec.dtype == dtp
        # fp32: the exact values; 16-bit: the exact values rounded once
        assert torch.equal(spec.cpu(), torch.from_numpy(want_spec).to(dtp)), (case, dtp, "spec")
        assert torch.equal(spat.cpu(), torch.from_numpy(want_spat).to(dtp)), (case, dtp, "spat")
    if case == "all_and_none":
        assert not want_spec[1].any() and np.array_equal(want_spat[1].reshape(F, T, 2, 2), x[1].transpose(1, 2, 3, 0))
        assert not want_spat[0].any()


def test_probe_mask_launch_flags_input_outside_fp16_range_like_mode_0():
    from sar_ssl_amd import hip
    dev = _dev()
    x, idx, ch = _mask_case("b1_f3_t5")
    mp = np.ones((1, 5), dtype=np.uint8)
    mp[0, idx[0]] = 0
    mpd, chd = torch.from_numpy(mp).to(dev), torch.from_numpy(ch.astype(np.int32)).to(dev)
    hip.fp16_overflow(clear=True)
    hip.mask_inputs(torch.from_numpy(x).to(dev), mpd, chd, 2, torch.float16)
    assert not hip.fp16_overflow(clear=True)
    big = x.copy()
    big[0, 1, 2, 1, 0] = 7.0e4                 # (the flag follows the input, whatever the masks hide - as in mode 0)
    for mode in (0, 2):
        hip.mask_inputs(torch.from_numpy(big).to(dev), mpd, chd, mode, torch.float16)
        assert hip.fp16_overflow(clear=True), mode
    hip.mask_inputs(torch.from_numpy(big).to(dev), mpd, chd, 2, torch.bfloat16)
    assert not hip.fp16_overflow(clear=True)


# ---------------------------------------------------------------- 2. one step against the reference (F17)
@pytest.mark.parametrize("prec", MODES)
def test_frozen_step_vs_reference(prec):
    """Fixture F17: one train-mode step of the reference's frozen stage at F3's shape.  Gates: parity.GATES[prec] - measured for these launches
    at this shape (F3)."""
    from sar_ssl_amd import hip, runtime
    from sar_ssl_amd.parity import GATES
    g = GATES[prec]
    z = _npz("f17_frozen_step.npz")
    gen = _generator()
    dev = _dev()
    tag = "frozen_step.%s." % prec
    runtime.set_precision(prec)
    try:
        B, T = int(z["B"]), int(z["T"])
        net, _ = _frozen_net(T, dev, int(z["weight_seed"]))
        net.to(dev).train()
        x = hip.stft_frontend(recipes.recipe_signal(B, int(z["nsample"]), 2, seed=int(z["sig_seed"])).to(dev))
        idx, ch = z["mask_idx"].astype(np.int64), z["mask_ch"].astype(np.int64)
        assert set(ch.tolist()) == {0, 1}
        net.set_masks(idx, ch)
        loss, diff, vis = net(x)
        loss.backward()
        check(tag + "loss", abs(loss.item() / float(z["loss"]) - 1), g["loss"])
        assert diff.item() == 0.0 and float(z["diff"]) == 0.0 and not diff.requires_grad
        # prediction at the masked frames: the rows the step's decoder ran on
        assert set(vis.keys()) == {"mask", "pred", "tar"}
        pred = vis["pred"]
        assert pred.shape == (B, 256, T, 2, 2)
        rows = pred.permute(0, 2, 1, 3, 4).reshape(B, T, -1)
        pred_m = torch.stack([rows[b, torch.from_numpy(idx[b]).to(dev)] for b in range(B)]).reshape(-1).cpu()
        n, seed = (int(v) for v in z["pred_sample"])
        got = pred_m[torch.from_numpy(gen.sample_idx(pred_m.numel(), n, seed))]
        want = torch.from_numpy(z["pred_vals"])
        check(tag + "pred", ((got - want).abs().max() / float(z["pred_absmax"])).item(), g["per_bin_max"])
        check(tag + "pred_rms", ((got - want).pow(2).mean().sqrt() / float(z["pred_absmax"])).item(), g["per_bin_rms"])
        # vis['mask'] / vis['tar']: exact
        mask = np.ones((B, 256, T, 2), dtype=np.float32)
        for b in range(B):
            mask[b, :, idx[b], ch[b]] = 0.0
        assert torch.equal(vis["mask"].cpu(), torch.from_numpy(mask))
        assert torch.equal(vis["tar"], x.permute(0, 2, 3, 4, 1))
        # gradients: the probe decoder's, nothing else
        gtol = g["grad_norm_body"] if prec == "hybrid" else g["grad_norm"]
        ns, sseed = (int(v) for v in z["grad_sample"])
        for k, p in net.named_parameters():
            if k.startswith(DEC):
                assert p.grad is not None, k
                ref = float(z["grad_norm." + k])
                check(tag + "gradnorm." + k, abs(p.grad.double().norm().item() - ref) / ref, gtol)
                gs = p.grad.reshape(-1).float().cpu()[torch.from_numpy(gen.sample_idx(p.numel(), ns, sseed))]
                print("GRADSAMPLE %s%s max deviation / max|g| = %.3e" % (tag, k, float((gs - torch.from_numpy(z["grad_vals." + k])).abs().max())
                                                                       / float(z["grad_absmax." + k])))
            else:
                assert p.grad is None or not bool(p.grad.any()), k
        assert [k for k, p in net.named_parameters() if not k.startswith(DEC)] == json.loads(str(z["nograd_json"]))
        # BatchNorm: train() mode - batch statistics, running statistics updated once
        sd = net.state_dict()
        off, man = 0, _manifest()
        for k in json.loads(str(z["bn_names_json"])):
            nel = int(np.prod(man[k]))
            check(tag + "bn." + k, _relerr(sd[k], z["bn_vals"][off:off + nel]), g["bn_running"])
            off += nel
        assert off == z["bn_vals"].size
        assert all(int(v) == 1 for k, v in sd.items() if k.endswith("num_batches_tracked"))
    finally:
        runtime.set_precision("bf16")


def test_frozen_step_masked_rows_eval_and_full_prediction(monkeypatch):
    """The training step runs the decoder on the masked frames' rows; vis['pred'] is formed on request and carries the step's own rows;
    `_full_pred_once` and eval / no_grad run the decoder on every frame; dropout is drawn in train() mode."""
    from sar_ssl_amd import engine, runtime
    dev = _dev()
    runtime.set_precision("fp16")
    calls = []
    orig = engine.decoder_fwd

    def recording(e, dec, saved):
        calls.append(orig(e, dec, saved))
        return calls[-1]
    monkeypatch.setattr(engine, "decoder_fwd", recording)
    try:
        T, B = 8, 3
        net, _ = _frozen_net(T, dev, 3)
        net.to(dev).train()
        x = torch.from_numpy(np.random.default_rng(3).standard_normal((B, 2, 256, T, 2)).astype(np.float32)).to(dev)
        idx, ch = np.array([[0, 2, 5, 7], [1, 2, 3, 4], [0, 1, 6, 7]]), np.array([0, 1, 1])
        rows = torch.from_numpy(idx).to(dev)
        pick = lambda p, r: torch.stack([p.permute(0, 2, 1, 3, 4).reshape(B, T, -1)[b, r[b]] for b in range(B)])
        net.set_masks(idx, ch)
        loss, diff, vis = net(x)
        assert len(calls) == 1 and calls[0].shape == (B * 4, 256 * 4)                # the decoder ran on the masked frames' rows only
        loss.backward()
        assert len(calls) == 1                                                      # ... and nothing was formed for vis yet
        g_compact = net.spec_spat_decoder.proj[2].weight.grad.clone()
        pred = vis["pred"]                                                          # on request: the decoder on every frame,
        assert len(calls) == 2 and calls[1].shape == (B * T, 256 * 4) and pred.shape == (B, 256, T, 2, 2)
        assert torch.equal(pick(pred, rows).reshape(B * 4, -1), calls[0].float())    # the step's own prediction at the masked frames
        other = torch.from_numpy(np.array([np.setdiff1d(np.arange(T), i) for i in idx])).to(dev)
        assert torch.equal(pick(pred, other), pick(calls[1].float().view(B, T, 256, 2, 2).permute(0, 2, 1, 3, 4), other))
        net.spec_spat_decoder.zero_grad(set_to_none=True)
        net.__dict__["_full_pred_once"] = True
        net.set_masks(idx, ch)
        loss_f, _, vis_f = net(x)
        assert len(calls) == 3 and calls[2].shape == (B * T, 256 * 4) and "_full_pred_once" not in net.__dict__
        loss_f.backward()
        # dropout 0: the same arithmetic on the same rows up to the summation order of a product with another row count
        assert abs(loss.item() / loss_f.item() - 1) < 1e-4
        assert _relerr(g_compact, net.spec_spat_decoder.proj[2].weight.grad.cpu().numpy()) < 2e-2
        assert _relerr(pick(pred, rows), pick(vis_f["pred"], rows).cpu().numpy()) < 2e-3 and len(calls) == 3
        # eval / no_grad: every frame, running statistics untouched
        net.eval()
        before = {k: v.clone() for k, v in net.state_dict().items()}
        with torch.no_grad():
            net.set_masks(idx, ch)
            loss_e, diff_e, vis_e = net(x)
        assert torch.isfinite(loss_e) and diff_e.item() == 0.0 and calls[-1].shape == (B * T, 256 * 4)
        assert all(torch.equal(v, before[k]) for k, v in net.state_dict().items())
        # train() with dropout on: the frozen encoders draw masks (two calls differ), eval does not
        net.train()
        _set_dropout(net, 0.1)
        out = []
        for _ in range(2):
            net.set_masks(idx, ch)
            out.append(net(x)[0].item())
        assert out[0] != out[1]
    finally:
        runtime.set_precision("bf16")


# ---------------------------------------------------------------- 3. the learner's epochs against the reference's (F18)
def _update_norms(net, init):
    return {k: float((p.detach().float().cpu().double() - init[k].double()).norm()) for k, p in net.named_parameters()}


@pytest.mark.parametrize("prec", MODES)
def test_frozen_epochs_vs_reference_pretrain_epoch(prec, monkeypatch):
    """Fixture F18: the reference's own pretrain_epoch x 2 (a new learning rate and a fresh Adam in the second) and one pretest_epoch on its
    frozen-stage model.  `upd`: the tolerance tests/test_gpu_train.py::test_pretrain_epoch_vs_reference_pretrain_epoch uses per mode."""
    from sar_ssl_amd import hip, runtime, synth
    from sar_ssl_amd.parity import GATES
    upd = {"fp32": 1e-2, "bf16": 2e-2, "fp16": 5e-3, "hybrid": 5e-3}[prec]
    z = _npz("f18_frozen_epochs.npz")
    dev = _dev()
    tag = "frozen_epochs.%s." % prec
    try:
        net, init = _frozen_net(256, dev, int(z["weight_seed"]))
        lrn = _learner(net)
        if prec != "fp32":
            lrn.amp(prec)
        nfrozen = lrn._flat.group_spans["decoder"][0]
        assert lrn._flat.frozen_ranges() == [(0, nfrozen)]
        at_adam, adam = [], hip.adam_step

        def adam_step(p, g, *a, **k):                                                # the frozen ranges of the gradient buffer when Adam runs
            at_adam.append(float(g[:nfrozen].abs().max()))
            return adam(p, g, *a, **k)
        monkeypatch.setattr(hip, "adam_step", adam_step)
        B, nb = int(z["B"]), int(z["nbatch"])
        pool = torch.from_numpy(synth.make_batch(int(z["sig_seed"]), B * nb))
        dataset = [[pool[i * B:(i + 1) * B]] for i in range(nb)]
        for e in (1, 2):
            random.seed(int(z["mask_seed"][e - 1]))
            assert not lrn._use_step_graph()
            loss, diff, vis = lrn.pretrain_epoch(dataset, lr=float(z["lr"][e - 1]), epoch=e)
            assert net.training == bool(z["training_flag"]) and "_step_graph" not in lrn.__dict__
            check(tag + "e%d.loss" % e, abs(loss / float(z["epoch%d.loss" % e]) - 1), GATES[prec]["loss"])
            assert diff == 0.0 and float(z["epoch%d.diff" % e]) == 0.0
            assert vis["pred"].shape == (B, 256, 256, 2, 2) and lrn.skipped_steps_last_epoch == 0
        assert at_adam == [0.0] * (2 * nb)
        ref = json.loads(str(z["update_norm_json"]))
        got = _update_norms(net, init)
        tot = lambda d: sum(v * v for v in d.values()) ** 0.5
        check(tag + "update_norm_total", abs(tot(got) / tot(ref) - 1), upd)
        moved = [k for k, v in got.items() if v > 0]
        assert moved == json.loads(str(z["moved_json"])) and all(k.startswith(DEC) for k in moved) and len(moved) == 4
        for k, p in net.named_parameters():                                          # encoders and the two unused decoders: bit for bit
            if not k.startswith(DEC):
                assert torch.equal(p.detach().cpu(), init[k]), k
        k = "spec_encoder.patch_embed.1.running_mean"
        assert bool(z["bn_moved"]) and not torch.equal(net.state_dict()[k].cpu(), init[k])      # train(): the frozen encoders' statistics move
        random.seed(int(z["val_mask_seed"]))
        lv, dv, _ = lrn.pretest_epoch(dataset)
        check(tag + "val.loss", abs(lv / float(z["val.loss"]) - 1), GATES[prec]["loss"])
        assert dv == 0.0 and not net.training
    finally:
        runtime.set_precision("bf16")


# ---------------------------------------------------------------- 4. / 5. guard and checkpoints
def test_trainable_encoder_parameter_is_refused():
    from sar_ssl_amd import runtime
    dev = _dev()
    runtime.set_precision("fp16")
    try:
        net, _ = _frozen_net(8, dev, 3)
        net.to(dev).train()
        x = torch.from_numpy(np.random.default_rng(4).standard_normal((2, 2, 256, 8, 2)).astype(np.float32)).to(dev)
        name = "spat_encoder.embed.layers.2.sequential.4.bias"
        dict(net.named_parameters())[name].requires_grad = True                      # flipped after construction, as the CLI flips them
        with pytest.raises(NotImplementedError, match=name.replace(".", r"\.")):
            net(x)
        with torch.no_grad():                                                        # no autograd: nothing to refuse
            assert torch.isfinite(net(x)[0])
        dict(net.named_parameters())[name].requires_grad = False
        loss, _, _ = net(x)
        loss.backward()
        assert torch.isfinite(loss)
    finally:
        runtime.set_precision("bf16")


def test_frozen_checkpoint_round_trip(tmp_path):
    from sar_ssl_amd import runtime, synth
    dev = _dev()
    try:
        T = 8
        net, init = _frozen_net(T, dev, 3)
        lrn = _learner(net)
        lrn.amp()
        data = torch.from_numpy(synth.make_batch(0, 4, nsample=512 + 256 * (T - 1)))
        loader = [[data[i:i + 2]] for i in (0, 2)]
        random.seed(0)
        loss, diff, _ = lrn.pretrain_epoch(loader, lr=1e-3, epoch=1)
        assert np.isfinite(loss) and diff == 0.0
        lv = lrn.pretest_epoch(loader)[0]
        best = lrn.is_best_epoch(-lv)
        lrn.save_checkpoint(epoch=1, checkpoints_dir=str(tmp_path), is_best_epoch=best)
        ck = torch.load(str(tmp_path / "best_model.tar"), map_location="cpu", weights_only=False)
        assert set(ck.keys()) == {"epoch", "max_score", "model"} and list(ck["model"].keys()) == list(_manifest().keys())
        assert not torch.equal(ck["model"][DEC + "proj.0.weight"], init[DEC + "proj.0.weight"])
        net2, _ = _frozen_net(T, dev, 5)
        lrn2 = _learner(net2)
        lrn2.resume_checkpoint(str(tmp_path), from_latest=True)
        assert lrn2.start_epoch == 2 and lrn2.max_score == lrn.max_score
        for (k, a), (_, b) in zip(net.state_dict().items(), net2.state_dict().items()):
            assert torch.equal(a, b), k
        # the encoders of a PRETRAINING checkpoint into the stage's key set (code/run_pretrain.py:357)
        man_pre = json.load(open(os.path.join(GOLD, "state_dict_manifest.json")))["pretrain"]
        pre = recipes.recipe_state_dict(man_pre, 7)
        torch.save({"epoch": 3, "max_score": -1.0, "model": pre}, str(tmp_path / "best_model.tar"))
        assert lrn2.load_checkpoint_best(str(tmp_path), as_all_state=False) == 3
        sd = net2.state_dict()
        for k, v in pre.items():
            if not k.startswith("decoder."):
                assert torch.equal(sd[k].cpu(), v), k
        assert torch.equal(sd[DEC + "proj.0.weight"], net.state_dict()[DEC + "proj.0.weight"])
    finally:
        runtime.set_precision("bf16")


# ---------------------------------------------------------------- 6. the command line
def _write_segments(work, sizes):
    from sar_ssl_amd import dataset, synth
    for split, n, base in sizes:
        d = work / "SAR-SSL" / "data" / "MicSig" / "simu" / split
        d.mkdir(parents=True)
        pcm = synth.to_pcm16(synth.make_batch(base, min(n, 32)))
        for i in range(n):
            dataset.write_wav_pcm16(str(d / ("%d.wav" % i)), np.roll(pcm[i % len(pcm)], 997 * (i // len(pcm)), axis=0))


def test_run_pretrain_frozen_encoder_entry_point(tmp_path):
    """`run_pretrain.py --pretrain-frozen-encoder --simu-exp` on top of a pretraining run's best_model.tar: one epoch of two steps + validation,
    scalars and checkpoints under exp/pretrain_frozen_encoder/<time>, encoders as loaded, a trained probe decoder."""
    from sar_ssl_amd import model
    work = tmp_path / "work"
    _write_segments(work, (("pretrain", 16, 0), ("preval", 8, 500)))
    man_pre = json.load(open(os.path.join(GOLD, "state_dict_manifest.json")))["pretrain"]
    pre = recipes.recipe_state_dict(man_pre, 0)
    pre_dir = work / "SAR-SSL" / "exp" / "pretrain" / "t0"
    pre_dir.mkdir(parents=True)
    torch.save({"epoch": 1, "max_score": -1.0, "model": pre}, str(pre_dir / "best_model.tar"))
    cmd = [sys.executable, os.path.join(ROOT, "run_pretrain.py"), "--pretrain-frozen-encoder", "--simu-exp", "--gpu-id", "0,", "--work-dir", str(work),
           "--bs", "8", "8", "8", "--nepoch", "1", "--workers", "2", "--time", "t0"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    logd = work / "SAR-SSL" / "exp" / "pretrain_frozen_encoder" / "t0"
    recs = [json.loads(l) for l in open(logd / "scalars.jsonl").read().strip().splitlines()]
    assert len(recs) == 1 and recs[0]["epoch"] == 1
    assert all(np.isfinite(recs[0][k]) for k in ("loss_train", "diff_train", "loss_val", "diff_val", "lr", "nparam_M"))
    assert recs[0]["diff_train"] == 0.0 and recs[0]["diff_val"] == 0.0
    assert (logd / "latest_model.tar").exists() and (logd / "best_model.tar").exists() and (logd / "config.json").exists()
    ck = torch.load(str(logd / "latest_model.tar"), map_location="cpu", weights_only=False)
    assert ck["epoch"] == 1 and list(ck["model"].keys()) == list(_manifest().keys())
    params = set(k for k in man_pre if not k.endswith(("running_mean", "running_var", "num_batches_tracked")))
    nenc = 0
    for k, v in pre.items():
        if k in params and not k.startswith("decoder."):
            assert torch.equal(ck["model"][k], v), k
            nenc += 1
    assert nenc > 100
    with torch.random.fork_rng():                                                 # the entry point seeds torch with --seed (1) and builds the model
        torch.manual_seed(1)
        fresh = model.SARSSL(sig_shape=(256, 256, 2, 2), pretrain=False, pretrain_frozen_encoder=True, device="cpu").state_dict()
    for k in fresh:
        if k.startswith(DEC):
            assert not torch.equal(ck["model"][k], fresh[k]), k
        elif k.startswith(("spec_decoder.", "spat_decoder.")):
            assert torch.equal(ck["model"][k], fresh[k]), k                          # the unused decoders: as initialised
