"""Fixtures of the frozen-encoder probe stage (``--pretrain-frozen-encoder``), from the REAL reference (build container only):

    python tools/make_golden_frozen.py [--only manifest,f17,f18]

Imports the reference through oracle/ref_shim.py and takes weights / signals from oracle/recipes.py; nothing of the reference's source
travels - the files hold numbers, seeds and names.

  tests/golden/state_dict_manifest_frozen.json   keys and shapes of SARSSL(pretrain=False, pretrain_frozen_encoder=True) at (256, 256, 2, 2)
  tests/golden/f17_frozen_step.npz                one train-mode step at B = 2, T = 256 (F3's shape, recipe weights seed 0, recipe signal
                                                  seed 3, dropout 0, encoders frozen the way the CLI freezes them) + the two encoder inputs of
                                                  a B = 3, T = 8 (F = 16) case, captured with forward pre-hooks
  tests/golden/f18_frozen_epochs.npz              the reference's own pretrain_epoch x 2 epochs x 2 batches of B = 2 and one pretest_epoch
"""
import argparse
import json
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "oracle"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import ref_shim                      # noqa: E402
import recipes                       # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
DEC = "spec_spat_decoder."
# F17: Python's RNG seed in front of the forward (both masked-channel values occur at B = 2); weight / signal recipe seeds as F3
F17 = dict(B=2, T=256, weight_seed=0, sig_seed=3, mask_seed=4322, nsample=65792)
# the small probe-input case (B = 3, T = 8): both masked-channel values occur
PROBE = dict(B=3, T=8, F=16, x_seed=977, mask_seed=21)
PRED_SAMPLE, GRAD_SAMPLE = (2048, 13), (48, 29)          # (entries, seed) of sample_idx: the tests regenerate the indices
F18 = dict(B=2, nbatch=2, T=256, weight_seed=0, sig_seed=2000, lr=[1e-3, 5e-4], mask_seed=[4100, 4101], val_mask_seed=4200)


def manifest_of(module):
    return {k: list(v.shape) for k, v in module.state_dict().items()}


def set_dropout(module, p):
    for m in module.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = p


def probe_x():
    """Input of the small probe-input case, (B, mic, F, T, reim) f32 from a stored seed."""
    p = PROBE
    return np.random.default_rng(p["x_seed"]).standard_normal((p["B"], 2, p["F"], p["T"], 2)).astype(np.float32)


def sample_idx(numel, n, seed):
    """n entry indices spread over range(numel) by a multiplicative hash of (k, seed): plain integer arithmetic, so the tests regenerate
    them on any machine (a repeated index is harmless)."""
    k = np.arange(min(n, numel), dtype=np.int64)
    return np.sort((k * 2654435761 + 40503 * seed) % numel)


def freeze_encoders(net):
    """What the reference's command line does after loading the encoders: every parameter whose name contains 'encoder'."""
    n = 0
    for k, p in net.named_parameters():
        if "encoder" in k:
            p.requires_grad = False
            n += 1
    return n


def build(ref_model, ref_learner, T, weight_seed):
    """(net, learner) of the reference's frozen stage: recipe weights, dropout 0, encoders frozen."""
    net = ref_model.SARSSL(sig_shape=(256, T, 2, 2), pretrain=False, pretrain_frozen_encoder=True, device="cpu")
    net.load_state_dict(recipes.recipe_state_dict(manifest_of(net), weight_seed))
    set_dropout(net, 0.0)
    freeze_encoders(net)
    lrn = ref_learner.STFTLearner(net, win_len=512, win_shift_ratio=0.5, nfft=512, fre_used_ratio=1, fs=16000, task=None, ch_mode="M")
    lrn.cpu()
    return net, lrn


def masks_of(vis_mask):
    """(idx (B, nm) ascending, ch (B)) from the reference's dense mask (B, F, T, mic), 0 = masked."""
    m = vis_mask
    ch = m[:, 0].sum(dim=1).argmin(dim=1)
    idx = torch.stack([(m[b, 0, :, int(ch[b])] == 0).nonzero().flatten() for b in range(m.shape[0])])
    return idx.numpy().astype(np.int64), ch.numpy().astype(np.int64)


def f17_step(ref_model, ref_learner):
    """One train-mode step of the reference's frozen stage -> (net, loss, diff, vis, x)."""
    c = F17
    net, lrn = build(ref_model, ref_learner, c["T"], c["weight_seed"])
    net.train()
    x, = lrn.data_preprocess(recipes.recipe_signal(c["B"], c["nsample"], 2, seed=c["sig_seed"]), None)
    random.seed(c["mask_seed"])
    loss, diff, vis = net(x)
    loss.backward()
    return net, loss, diff, vis, x


def f_manifest(ref_model):
    net = ref_model.SARSSL(sig_shape=(256, 256, 2, 2), pretrain=False, pretrain_frozen_encoder=True, device="cpu")
    with open(os.path.join(GOLD, "state_dict_manifest_frozen.json"), "w") as f:
        json.dump({"frozen": manifest_of(net), "nparams_frozen": int(sum(p.numel() for p in net.parameters()))}, f, indent=0)


def f17(ref_model, ref_learner):
    c = F17
    net, loss, diff, vis, _ = f17_step(ref_model, ref_learner)
    idx, ch = masks_of(vis["mask"])
    assert len(set(ch.tolist())) == 2, "choose a mask seed whose masked channels differ"
    B, T, nm = c["B"], c["T"], idx.shape[1]
    pred = vis["pred"].permute(0, 2, 1, 3, 4).contiguous().view(B, T, -1)               # (B, T, F*reim*mic)
    pred_m = torch.stack([pred[b, torch.from_numpy(idx[b])] for b in range(B)])           # rows of the masked frames, ascending
    sidx = sample_idx(pred_m.numel(), *PRED_SAMPLE)
    store = {k: np.int64(v) for k, v in c.items()}
    store.update({"mask_idx": idx.astype(np.int16), "mask_ch": ch.astype(np.int16), "loss": np.float64(loss.item()), "diff": np.float64(diff.item()),
                  "pred_sample": np.array(PRED_SAMPLE), "pred_vals": pred_m.reshape(-1)[sidx].numpy(), "pred_absmax": np.float64(pred_m.abs().max()),
                  "grad_sample": np.array(GRAD_SAMPLE)})
    nograd = []
    for k, p in net.named_parameters():
        if p.grad is None:
            nograd.append(k)
            continue
        assert k.startswith(DEC), k
        g = p.grad.reshape(-1)
        si = sample_idx(g.numel(), *GRAD_SAMPLE)
        store["grad_norm." + k] = np.float64(g.double().norm())
        store["grad_absmax." + k] = np.float64(g.abs().max())
        store["grad_vals." + k] = g[si].numpy().copy()
    store["nograd_json"] = np.array(json.dumps(nograd))
    bn = [(k, v.numpy().reshape(-1)) for k, v in net.state_dict().items() if k.endswith(("running_mean", "running_var"))]
    store["bn_names_json"] = np.array(json.dumps([k for k, _ in bn]))            # one array, split by the manifest's shapes
    store["bn_vals"] = np.concatenate([v for _, v in bn])
    # ---- the two encoder inputs of a small case, as the reference's forward hands them over
    # (B = 3, T = 8, F = 16; the model calls its encoders' .forward directly, which runs no hooks: the hook sits on each encoder's first
    #  module, the CNN stem, which receives the encoder input as (B, reim*2 + mic, F, T) - stored channels-last, (B, F, T, 4))
    p = PROBE
    net = ref_model.SARSSL(sig_shape=(p["F"], p["T"], 2, 2), patch_shape=(p["F"], 1), pretrain=False, pretrain_frozen_encoder=True, device="cpu")
    net.train()
    got = {}
    hooks = [getattr(net, n).patch_embed.register_forward_pre_hook(
        lambda mod, args, n=n: got.__setitem__(n, args[0].detach().permute(0, 2, 3, 1).contiguous().clone())) for n in ("spec_encoder", "spat_encoder")]
    random.seed(p["mask_seed"])
    _, _, pvis = net(torch.from_numpy(probe_x()))
    for h in hooks:
        h.remove()
    pidx, pch = masks_of(pvis["mask"])
    assert len(set(pch.tolist())) == 2
    store.update({"probe.mask_idx": pidx.astype(np.int16), "probe.mask_ch": pch.astype(np.int16), "probe.spec_in": got["spec_encoder"].numpy(),
                  "probe.spat_in": got["spat_encoder"].numpy(), "probe.x_seed": np.int64(p["x_seed"]), "probe.mask_seed": np.int64(p["mask_seed"])})
    print("f17 loss", loss.item(), "diff", diff.item(), "masked channels", ch.tolist(), "/", pch.tolist(), "no grad:", len(nograd), flush=True)
    np.savez_compressed(os.path.join(GOLD, "f17_frozen_step.npz"), **store)


def f18(ref_model, ref_learner):
    from sar_ssl_amd import synth
    c = F18
    net, lrn = build(ref_model, ref_learner, c["T"], c["weight_seed"])
    init = {k: v.detach().clone() for k, v in net.state_dict().items()}
    B, nb = c["B"], c["nbatch"]
    pool = torch.from_numpy(synth.make_batch(c["sig_seed"], B * nb))
    dataset = [[pool[i * B:(i + 1) * B]] for i in range(nb)]
    store = {"B": B, "nbatch": nb, "sig_seed": c["sig_seed"], "weight_seed": c["weight_seed"], "lr": np.array(c["lr"]),
             "mask_seed": np.array(c["mask_seed"]), "val_mask_seed": c["val_mask_seed"]}
    for e in range(2):
        random.seed(c["mask_seed"][e])
        loss, diff, _ = lrn.pretrain_epoch(dataset, lr=c["lr"][e], epoch=e + 1)
        store["epoch%d.loss" % (e + 1)] = np.float64(loss)
        store["epoch%d.diff" % (e + 1)] = np.float64(diff)
        print("frozen pretrain_epoch", e + 1, loss, diff, flush=True)
    store["training_flag"] = np.int64(net.training)
    upd = {k: float((p.detach() - init[k]).double().norm()) for k, p in net.named_parameters()}
    store["update_norm_json"] = np.array(json.dumps(upd))
    store["moved_json"] = np.array(json.dumps([k for k, v in upd.items() if v > 0]))
    store["bn_moved"] = np.int64(not torch.equal(net.state_dict()["spec_encoder.patch_embed.1.running_mean"],
                                                 init["spec_encoder.patch_embed.1.running_mean"]))
    random.seed(c["val_mask_seed"])
    lv, dv, _ = lrn.pretest_epoch(dataset)
    store["val.loss"], store["val.diff"] = np.float64(lv), np.float64(dv)
    print("frozen pretest_epoch", lv, dv, "moved:", json.loads(str(store["moved_json"])), flush=True)
    np.savez_compressed(os.path.join(GOLD, "f18_frozen_epochs.npz"), **store)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    torch.manual_seed(0)
    torch.set_num_threads(8)
    ref_model, ref_learner, _ = ref_shim.load()
    todo = a.only.split(",") if a.only else ["manifest", "f17", "f18"]
    if "manifest" in todo: f_manifest(ref_model)
    if "f17" in todo: f17(ref_model, ref_learner)
    if "f18" in todo: f18(ref_model, ref_learner)
    print("frozen-stage fixtures written to", GOLD)
