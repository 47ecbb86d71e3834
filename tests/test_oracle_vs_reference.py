"""The oracle against the reference's own forward + backward of one small pretraining step, stored as fixture F16
(oracle/make_golden.py: front-end output, loss, diff and, per parameter, the gradient's largest magnitude, its norm and 48 sampled
entries - all of them for smaller tensors)."""
import json
import os
import random

import numpy as np
import torch

import recipes
import sarssl_oracle as orc
from conftest import GOLD


def test_oracle_matches_reference_small_pretrain_step():
    z = np.load(os.path.join(GOLD, "f16_small_step.npz"), allow_pickle=False)
    B, T = int(z["B"]), int(z["T"])
    man = json.load(open(os.path.join(GOLD, "state_dict_manifest.json")))["pretrain"]
    sig = recipes.recipe_signal(B, 512 + 256 * (T - 1), 2, seed=int(z["sig_seed"]))
    x_ref = torch.from_numpy(z["x"])
    x = orc.data_preprocess(sig)
    assert torch.allclose(x, x_ref, rtol=1e-5, atol=1e-6)
    random.seed(int(z["mask_seed"]))
    idx, ch = orc.gen_masks(B, T, T // 2, 2, random)
    loss_ref, diff_ref = float(z["loss"]), float(z["diff"])
    osd = recipes.recipe_state_dict(man, int(z["weight_seed"]))
    params = {k: v.requires_grad_(True) for k, v in osd.items() if orc.is_param(k)}
    loss, diff, _ = orc.sarssl_pretrain_forward(x, osd, idx, ch, train=True, p_drop=0.0)
    loss.backward()
    assert abs(loss.item() / loss_ref - 1) < 1e-5 and abs(diff.item() / diff_ref - 1) < 1e-6
    names = json.loads(str(z["names_json"]))
    assert sorted(names) == sorted(params)
    offs, sidx, svals, gmax, gnorm = z["sample_offsets"], z["sample_idx"], z["sample_vals"], z["grad_absmax"], z["grad_norm"]
    top = float(gmax.max())
    for i, k in enumerate(names):
        ref = torch.from_numpy(svals[offs[i]:offs[i + 1]])
        got_all = params[k].grad.reshape(-1)
        got = got_all[torch.from_numpy(sidx[offs[i]:offs[i + 1]].astype(np.int64))]
        scale = max(float(gmax[i]), 1e-6 * top)      # analytically-zero grads (key bias) are round-off on both sides
        assert (got - ref).abs().max().item() / scale < 1e-2, k          # tiny batch (6144 stem pixels): f32 summation-order noise through BatchNorm
        assert abs(got_all.abs().max().item() - float(gmax[i])) / scale < 1e-2, k      # the tensor's largest entry, wherever it lies
        nscale = max(float(gnorm[i]), 1e-6 * top * got_all.numel() ** 0.5)
        assert abs(got_all.double().norm().item() - float(gnorm[i])) / nscale < 1e-2, k   # and every entry, through the norm
