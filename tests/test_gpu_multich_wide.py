"""GPU: SARSSL_MultiCH (code/model.py:793-821) with five or more mic pairs.  Its head is LayerNorm(256 * nmic_pair): wider than 1024 from
5 pairs on (4 mics under 'MM': 6 pairs, d = 1536; 8 mics under 'MM': 28 pairs, d = 7168), where sarssl_layernorm_fwd / _bwd run their
one-workgroup-per-row path.  Checked at the kernel (against f64 torch), the head (against the same torch modules in f64) and the model
(forward against the oracle, training steps against the oracle's autograd)."""
import copy

import pytest
import torch
import torch.nn.functional as F

import recipes
import sarssl_oracle as orc
from conftest import check
from test_gpu_downstream import TOL, _set_dropout

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


# ---------------------------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("d", [1028, 1280, 1536, 4096, 7168])
def test_wide_layernorm_kernels_match_f64(d, dtype):
    """sarssl_layernorm_fwd / _bwd at d > 1024: strided rows (ldx > d), with and without resid, dgamma / dbeta accumulated into non-zero
    buffers, M = 333 spread over several partial rows; the partials-only call + sarssl_ln_param_reduce_multi gives the direct call's
    dgamma / dbeta."""
    from sar_ssl_amd import hip
    tag = "lnwide.%d.%s" % (d, "f32" if dtype == torch.float32 else "bf16")
    # f32: the gate of the downstream-head test; bf16 storage of y / dx rounds by up to half a bf16 ulp, 2^-8 of the value (3.9e-3;
    # measured up to 3.4e-3 of the maximum)
    tol16 = 1e-5 if dtype == torch.float32 else 8e-3
    g = torch.Generator(device="cpu").manual_seed(d)
    gamma = (1 + 0.2 * torch.randn(d, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(d, generator=g)).to(DEV)
    worst = dict(y=0.0, stats=0.0, dx=0.0, dxr=0.0, param=0.0)
    for M in (1, 5, 64, 333):
        xs = (1.5 + 2.0 * torch.randn(M, d + 12, generator=g)).to(DEV, dtype)[:, :d]     # ldx = d + 12, a non-zero row mean
        assert xs.stride(0) == d + 12
        dy = torch.randn(M, d, generator=g).to(DEV, dtype)
        res = torch.randn(M, d, generator=g).to(DEV, dtype)
        y, stats = hip.layernorm_fwd(xs, gamma, beta, 1e-5)
        xr = xs.double().requires_grad_(True)
        gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
        yr = F.layer_norm(xr, (d,), gr, br, 1e-5)
        (yr * dy.double()).sum().backward()
        mu = xs.double().mean(dim=1)
        rs = 1.0 / torch.sqrt(((xs.double() - mu[:, None]) ** 2).mean(dim=1) + 1e-5)
        worst["y"] = max(worst["y"], _rel(y, yr.detach()))
        worst["stats"] = max(worst["stats"], _rel(stats[0], mu), _rel(stats[1], rs))
        dg0 = torch.randn(d, generator=g).to(DEV)
        db0 = torch.randn(d, generator=g).to(DEV)
        for resid in (None, res):
            dg, db = dg0.clone(), db0.clone()
            dx = hip.layernorm_bwd(dy, xs, gamma, stats, resid=resid, dgamma=dg, dbeta=db)
            want = xr.grad if resid is None else xr.grad + res.double()
            worst["dx" if resid is None else "dxr"] = max(worst["dx" if resid is None else "dxr"], _rel(dx, want))
            worst["param"] = max(worst["param"], _rel(dg - dg0, gr.grad), _rel(db - db0, br.grad))
            dg2, db2 = dg0.clone(), db0.clone()
            with hip.ln_reduce_batched():                # partials only, folded at exit by sarssl_ln_param_reduce_multi
                dx2 = hip.layernorm_bwd(dy, xs, gamma, stats, resid=resid, dgamma=dg2, dbeta=db2)
            assert torch.equal(dx2, dx) and torch.equal(dg2, dg) and torch.equal(db2, db), (M, resid is None)
            assert torch.equal(hip.layernorm_bwd(dy, xs, gamma, stats, resid=resid), dx)          # no parameter gradients
    for k in ("y", "dx", "dxr"):
        check("%s.%s" % (tag, k), worst[k], tol16)
    check("%s.stats" % tag, worst["stats"], 1e-5)
    check("%s.param" % tag, worst["param"], 1e-5)


# ---------------------------------------------------------------------------------------------------------------- head
@pytest.mark.parametrize("out", ["pairs", "one"])
@pytest.mark.parametrize("npair", [5, 6, 28])
def test_multich_head_wide_matches_torch_f64(npair, out):
    """pool_mean + head_apply on SARSSL_MultiCH.head_mch (LayerNorm(256 n), Linear, ReLU, Linear(., n | 1)): y, the input gradient and
    every parameter gradient against the same modules in f64."""
    from sar_ssl_amd import _lib, autograd as ag
    torch.manual_seed(npair)
    d, nout = 256 * npair, (npair if out == "pairs" else 1)
    seq = torch.nn.Sequential(torch.nn.LayerNorm(d), torch.nn.Linear(d, d), torch.nn.ReLU(), torch.nn.Linear(d, nout))
    with torch.no_grad():
        seq[0].weight.uniform_(0.8, 1.2)
        seq[0].bias.uniform_(-0.05, 0.05)
    seq = seq.to(DEV)
    ref = copy.deepcopy(seq).double()
    B, T = 3, 7
    emb = torch.randn(B * npair, T, 256, device=DEV, requires_grad=True)
    embr = emb.detach().double().requires_grad_(True)
    n0 = _lib.ncalls
    y = ag.head_apply(seq, ag.pool_mean(emb).reshape(B, d))
    assert _lib.ncalls - n0 >= 4                                          # library launches: mean, LayerNorm, two Linear
    gy = torch.randn_like(y)
    (y * gy).sum().backward()
    yr = ref(embr.mean(dim=1).reshape(B, d))
    (yr * gy.double()).sum().backward()
    tag = "headwide.%d.%d" % (npair, nout)
    check(tag + ".y", _rel(y, yr), 1e-5)
    check(tag + ".dx", _rel(emb.grad, embr.grad), 1e-5)
    for (k, p), (_, pr) in zip(seq.named_parameters(), ref.named_parameters()):
        check("%s.grad.%s" % (tag, k), _rel(p.grad, pr.grad), 2e-5)


# ---------------------------------------------------------------------------------------------------------------- model
NPAIR, NT, NSAMPLE = 6, 32, 8448                 # 4 mics, every pair ('MM'); nt = (8448 - 512) / 256 + 1 = 32


def _multich(task, seed=11):
    from sar_ssl_amd import model
    mch = model.SARSSL_MultiCH(sig_shape=(256, NT, 2, 2), nmic_pair=NPAIR, task=task, device=DEV)
    man = {k: list(v.shape) for k, v in mch.state_dict().items()}
    sd = recipes.recipe_state_dict(man, seed)
    mch.load_state_dict(sd)
    return mch.cuda(), sd


@pytest.mark.parametrize("prec", ["fp32", "hybrid"])
@pytest.mark.parametrize("task", ["TDOA", "DRR"])
def test_multich_six_pairs_forward_vs_oracle(task, prec):
    """4-mic signals -> fused front-end in 'MM' mode (6 pairs per segment) -> SARSSL_MultiCH(nmic_pair = 6), eval mode, against
    oracle.sarssl_multich_forward on oracle.data_preprocess(ch_mode='MM')."""
    from sar_ssl_amd import hip, runtime
    tol = 1e-3 if prec == "fp32" else TOL[prec]["pred"]
    B = 2
    sig = recipes.recipe_signal(B, NSAMPLE, 4, seed=4)
    mch, sd = _multich(task)
    mch.eval()
    runtime.set_precision(prec)
    try:
        with torch.no_grad():
            x = hip.stft_frontend(sig.to(DEV), ch_mode="MM")
            assert tuple(x.shape) == (B * NPAIR, 2, 256, NT, 2)
            pred, emb = mch(x)
    finally:
        runtime.set_precision("bf16")
    with torch.no_grad():
        pred_r, emb_r = orc.sarssl_multich_forward(orc.data_preprocess(sig, ch_mode="MM"), dict(sd), NPAIR)
    assert tuple(pred.shape) == (B, NPAIR if task == "TDOA" else 1) and tuple(emb.shape) == (B, 256 * NPAIR)
    check("multich6.%s.%s.pred" % (task, prec), _rel(pred.cpu(), pred_r), tol)
    check("multich6.%s.%s.embed" % (task, prec), _rel(emb.cpu(), emb_r), tol)


def _drr_learner(prec):
    from sar_ssl_amd import learner, runtime
    mch, sd = _multich("DRR", seed=13)
    _set_dropout(mch, 0.0)
    lrn = learner.STFTLearner(mch, win_len=512, win_shift_ratio=0.5, nfft=512, fre_used_ratio=1, fs=16000, task="DRR", ch_mode="MM")
    lrn.cuda()
    if prec == "fp32":
        runtime.set_precision("fp32")
    else:
        lrn.amp(prec)
    mch.train()
    B = 3
    sig = recipes.recipe_signal(B, NSAMPLE, 4, seed=8)
    drr = torch.tensor([4.0, -2.0, 7.5])
    return mch, sd, lrn, sig, drr


def _oracle_gradnorms(sd, sig, tar):
    """Autograd of the oracle's SARSSL_MultiCH in train mode (batch statistics, no dropout) with the learner's MSE loss."""
    sd = {k: v.clone() for k, v in sd.items()}
    params = {k: v.requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and orc.is_param(k)}
    v = orc.data_preprocess(sig, ch_mode="MM").permute(0, 3, 2, 4, 1)
    e = orc.embed_encoder(v, sd, "model_sch.spat_encoder.", 3, True, p_drop=0.0).mean(dim=1)
    e = e.reshape(-1, NPAIR * e.shape[-1])
    h = F.layer_norm(e, (e.shape[-1],), sd["head_mch.0.weight"], sd["head_mch.0.bias"], orc.EPS_LN)
    h = F.relu(F.linear(h, sd["head_mch.1.weight"], sd["head_mch.1.bias"]))
    pred = F.linear(h, sd["head_mch.3.weight"], sd["head_mch.3.bias"])
    F.mse_loss(pred, tar).backward()
    return {k: float(p.grad.double().norm()) for k, p in params.items() if p.grad is not None}


def _steps(lrn, mch, sig, drr, n=5, lr=1e-4):
    from sar_ssl_amd import runtime
    opt = runtime.FusedAdam(lrn._flat, lr=lr)
    opt.zero_grad()
    x, tar = lrn.data_preprocess(sig, {"DRR": drr})
    losses = []
    for _ in range(n):
        pred, _ = mch(x)
        loss = lrn.loss(pred_batch=pred, gt_batch=tar)
        loss.backward()
        opt.step()
        opt.zero_grad()
        losses.append(float(loss.detach()))
    torch.cuda.synchronize()
    return losses


def test_multich_six_pairs_training_fp32_vs_oracle():
    """STFTLearner('MM', task 'DRR') + SARSSL_MultiCH(nmic_pair = 6), fp32: step-1 per-parameter gradient norms against the oracle's
    autograd, then Adam steps on one batch - the loss falls and every parameter stays finite."""
    from sar_ssl_amd import runtime
    try:
        mch, sd, lrn, sig, drr = _drr_learner("fp32")
        x, tar = lrn.data_preprocess(sig, {"DRR": drr})
        assert tuple(x.shape) == (3 * NPAIR, 2, 256, NT, 2) and tuple(tar.shape) == (3, 1)
        pred, _ = mch(x)
        lrn.loss(pred_batch=pred, gt_batch=tar).backward()
        refs = _oracle_gradnorms(sd, sig, tar.cpu())
        assert any(k.startswith("head_mch.") for k in refs) and any(k.startswith("model_sch.spat_encoder.") for k in refs)
        top = max(refs.values())
        worst, wk = 0.0, None
        for k, p in mch.named_parameters():
            if k not in refs:
                assert p.grad is None or float(p.grad.abs().max()) == 0.0, k         # unused branch (spec encoder)
                continue
            got = float(p.grad.double().norm())
            if refs[k] < 1e-6 * top:                                               # analytically zero (key-projection bias)
                assert got < 1e-4 * top, (k, got, refs[k])
            elif abs(got - refs[k]) / refs[k] > worst:
                worst, wk = abs(got - refs[k]) / refs[k], k
        check("multich6.train.fp32.gradnorm[worst=%s]" % wk, worst, TOL["fp32"]["grad"])
        losses = _steps(lrn, mch, sig, drr)
        print("multich6.train.fp32 losses", losses)
        assert losses[-1] < 0.2 * losses[0], losses          # measured: 21.3 -> 1.04
        assert all(bool(torch.isfinite(p).all()) for p in mch.parameters())
    finally:
        runtime.set_precision("bf16")


def test_multich_six_pairs_training_hybrid_loss_falls():
    from sar_ssl_amd import runtime
    try:
        mch, sd, lrn, sig, drr = _drr_learner("hybrid")
        losses = _steps(lrn, mch, sig, drr)
        print("multich6.train.hybrid losses", losses)
        assert losses[-1] < 0.2 * losses[0], losses          # measured: 21.3 -> 1.06
        assert all(bool(torch.isfinite(p).all()) for p in mch.parameters())
    finally:
        runtime.set_precision("bf16")
