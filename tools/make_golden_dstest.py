"""Fixture F19 of the downstream test stage (``run_downstream.py --ds-test``), from the REAL reference (build container only):

    python tools/make_golden_dstest.py

Imports the reference through oracle/ref_shim.py, takes weights from oracle/recipes.py and signals from sar_ssl_amd.synth, runs on the
CPU; nothing of the reference's source travels - the file holds numbers and seeds.  The seeds and batch splits below are what the tests
import; the checkpoints the tests need are rebuilt from the recipe seeds (``states``), no weights are stored.

  tests/golden/f19_dstest.npz
    tdoa.*     SARSSL((256, 64, 2, 2), pretrain=False, 'all', 'mlp', 'spat', 1); two recipe states saved as model1.tar / model2.tar with the
               reference's save_checkpoint, its ensembling([1, 2]), load_checkpoint_ensemble, test_epoch(return_metric, return_vis) over
               37 segments of 16 640 samples in batches of 16, 16 and 5: loss, metric, embed (37, 256), label, and the f64 sum / abs-sum of
               three ensemble tensors (ENSEMBLE_KEYS)
    t60.*      SARSSL((256, 256, 2, 2), ..., 'spec_spat', 1), one recipe state, 7 segments of 65 792 samples in batches of 4 and 3:
               test_epoch loss, metric, embed (7, 768), label
    wo_info.*  the reference's mae_wotrain seven numbers for task TDOA (40 training labels, the 37 test labels) and for task T60
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "oracle"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import recipes                       # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
# num_batches_tracked is 0 in every recipe state; nbt gives the two epochs' BatchNorm counters distinct values whose mean is whole, so that
# the reference's float average (long * 1/2) stands for an integer
TDOA = dict(T=64, embed="spat", nsample=16640, n=37, splits=((0, 16), (16, 32), (32, 37)), weight_seeds=(5, 6), nbt=(10, 20), sig_seed=300,
            label_seed=19, label_range=(-5e-4, 5e-4), task="TDOA", ntrain=40, train_label_seed=20)
T60 = dict(T=256, embed="spec_spat", nsample=65792, n=7, splits=((0, 4), (4, 7)), weight_seeds=(7,), nbt=(0,), sig_seed=400,
           label_seed=21, label_range=(0.2, 1.0), task="T60", ntrain=40, train_label_seed=22)
ENSEMBLE_KEYS = ("spat_encoder.patch_embed.0.weight", "spat_encoder.patch_embed.1.running_var", "spat_encoder.patch_embed.1.num_batches_tracked")
WO_INFO_NAMES = ("mae_test", "min_test", "max_test", "mae", "mean", "min", "max")


def manifest_of(module):
    return {k: list(v.shape) for k, v in module.state_dict().items()}


def build_net(model_module, c, device="cpu"):
    return model_module.SARSSL(sig_shape=(256, c["T"], 2, 2), pretrain=False, device=device, downstream_token="all", downstream_head="mlp",
                               downstream_embed=c["embed"], downstream_dlabel=1)


def states(manifest, c):
    """The recipe state dicts of case ``c``, one per weight seed, BatchNorm counters set to ``c['nbt']``."""
    out = []
    for seed, nbt in zip(c["weight_seeds"], c["nbt"]):
        sd = recipes.recipe_state_dict(manifest, seed)
        for k in sd:
            if k.endswith("num_batches_tracked"):
                sd[k] = torch.tensor(nbt, dtype=torch.int64)
        out.append(sd)
    return out


def labels(c, train=False):
    n, seed = (c["ntrain"], c["train_label_seed"]) if train else (c["n"], c["label_seed"])
    return torch.from_numpy(np.random.default_rng(seed).uniform(*c["label_range"], size=(n,)).astype(np.float32))


def label_loader(c, train=False, bs=16):
    """Batches whose first item is never read (mae_wotrain takes the second one only)."""
    lab = labels(c, train)
    return [(None, {c["task"]: lab[i:i + bs]}) for i in range(0, len(lab), bs)]


def loader(c):
    """The case's batches, (signal (b, nsample, 2) f32, {task: label (b,)}), on the CPU."""
    from sar_ssl_amd import synth
    sig = torch.from_numpy(synth.make_batch(c["sig_seed"], c["n"], nsample=c["nsample"]))
    lab = labels(c)
    return [(sig[a:b].contiguous(), {c["task"]: lab[a:b]}) for a, b in c["splits"]]


def _ref_learner(ref_model, ref_learner, c):
    net = build_net(ref_model, c)
    lrn = ref_learner.STFTLearner(net, win_len=512, win_shift_ratio=0.5, nfft=512, fre_used_ratio=1, fs=16000, task=c["task"], ch_mode="M")
    lrn.cpu()
    return net, lrn


def _check_manifest(net, c):
    """The build's model has the reference's keys and shapes, so the tests may take the manifest from it."""
    from sar_ssl_amd import model
    assert manifest_of(build_net(model, c)) == manifest_of(net), "state_dict keys / shapes differ from the reference's"


def f19(ref_model, ref_learner):
    store = {}
    # ---- tdoa: two epochs -> ensemble -> load -> test_epoch
    c = TDOA
    net, lrn = _ref_learner(ref_model, ref_learner, c)
    _check_manifest(net, c)
    with tempfile.TemporaryDirectory() as d:
        for epoch, sd in enumerate(states(manifest_of(net), c), start=1):
            net.load_state_dict(sd)
            lrn.save_checkpoint(epoch=epoch, checkpoints_dir=d, is_best_epoch=False, save_extra_hist=True)
        lrn.ensembling(checkpoints_dir=d, epochs=[1, 2])
        saved = torch.load(os.path.join(d, "ensemble_model.tar"), map_location="cpu", weights_only=False)
        assert saved["epoch"] == [1, 2]
        net2, lrn2 = _ref_learner(ref_model, ref_learner, c)
        lrn2.load_checkpoint_ensemble(checkpoints_dir=d)
    for k in ENSEMBLE_KEYS:
        v = net2.state_dict()[k].double()
        store["tdoa.sum." + k], store["tdoa.abssum." + k] = np.float64(v.sum()), np.float64(v.abs().sum())
    store["tdoa.saved_nbt_is_float"] = np.int64(saved["model"][ENSEMBLE_KEYS[2]].is_floating_point())
    loss, metric, vis = lrn2.test_epoch(loader(c), return_metric=True, return_vis=True)
    store.update({"tdoa.loss": np.float64(loss), "tdoa.metric": np.float64(float(metric)), "tdoa.embed": vis["embed"].numpy().astype(np.float32),
                  "tdoa.label": vis["label"].numpy().astype(np.float32)})
    print("tdoa test_epoch", loss, float(metric), vis["embed"].shape, flush=True)
    # ---- t60: nt = 256, both encoders' embeddings
    c = T60
    net, lrn = _ref_learner(ref_model, ref_learner, c)
    _check_manifest(net, c)
    net.load_state_dict(states(manifest_of(net), c)[0])
    loss, metric, vis = lrn.test_epoch(loader(c), return_metric=True, return_vis=True)
    store.update({"t60.loss": np.float64(loss), "t60.metric": np.float64(float(metric)), "t60.embed": vis["embed"].numpy().astype(np.float32),
                  "t60.label": vis["label"].numpy().astype(np.float32)})
    print("t60 test_epoch", loss, float(metric), vis["embed"].shape, flush=True)
    # ---- the no-information baseline
    for c in (TDOA, T60):
        _, lrn = _ref_learner(ref_model, ref_learner, dict(c, T=8))
        seven = lrn.mae_wotrain(label_loader(c, train=True), label_loader(c))
        store["wo_info." + c["task"]] = np.array(seven, dtype=np.float64)
        print("wo_info", c["task"], seven, flush=True)
    np.savez_compressed(os.path.join(GOLD, "f19_dstest.npz"), **store)


if __name__ == "__main__":
    import ref_shim
    torch.manual_seed(0)
    torch.set_num_threads(8)
    ref_model, ref_learner, _ = ref_shim.load()
    f19(ref_model, ref_learner)
    print("downstream test-stage fixture written to", GOLD)
