"""GPU: sarssl_regress_loss (csrc/head.hip) - the downstream learner's loss, metric and gradient in one launch - against an f64
restatement on the host: out = [mean (p - t)^2, mean |p - t|], dpred = 2 (p - t) / (B L), the running sums, the non-finite flag."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (B, L): one element, less than a wave, a ragged wave, one full wave, several waves with L > 1, more elements than the workgroup has threads
SHAPES = [(1, 1), (4, 1), (5, 3), (64, 1), (70, 6), (300, 1)]


def _data(B, L, seed):
    rng = np.random.default_rng(seed)
    pred = (rng.standard_normal((B, L)) * 3.0).astype(np.float32)
    tgt = (rng.standard_normal((B, L)) * 8.0).astype(np.float32)           # (TDOA targets are a few samples)
    return pred, tgt


def _ref(pred, tgt):
    d = pred.astype(np.float64) - tgt.astype(np.float64)
    return np.array([np.mean(d * d), np.mean(np.abs(d))]), 2.0 * d / d.size


def _ulp(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("B,L", SHAPES)
def test_regress_loss_against_f64(B, L):
    from sar_ssl_amd import hip
    dev = torch.device("cuda:0")
    keep = torch.zeros(2, dtype=torch.float32, device=dev)
    acc = torch.zeros(3, dtype=torch.float64, device=dev)
    outs = []
    for call, seed in enumerate((B * 31 + L, B * 31 + L + 1000)):
        pred, tgt = _data(B, L, seed)
        p, t = torch.from_numpy(pred).to(dev), torch.from_numpy(tgt).to(dev)
        out, dpred = hip.regress_loss(p, t, sink=(keep, acc), with_grad=True, skip_nonfinite=True)
        ref, dref = _ref(pred, tgt)
        got = out.cpu().numpy().astype(np.float64)
        print("regress_loss (%d, %d) call %d: out rel err %s" % (B, L, call, np.abs(got - ref) / ref))
        # an f64 sum rounded once to f32 plus one division: 2^-22 relative
        assert (np.abs(got - ref) <= 2.0 ** -22 * ref).all(), (got, ref)
        assert torch.equal(keep, out)
        dg = dpred.cpu().numpy().astype(np.float64)
        assert dg.shape == (B, L)
        assert (np.abs(dg - dref) <= _ulp(dref)).all(), np.abs(dg - dref).max()
        outs.append(got)
        # with dpred NULL nothing else changes
        acc2 = torch.zeros(3, dtype=torch.float64, device=dev)
        out2 = hip.regress_loss(p, t, sink=(None, acc2), skip_nonfinite=True)
        assert torch.equal(out2, out)
        assert acc2.cpu().tolist() == [float(got[0]), float(got[1]), 1.0]
    # acc after two calls = the f64 sum of the two (of the f32 words the calls wrote), count 2
    a = acc.cpu().numpy()
    assert a[0] == outs[0][0] + outs[1][0] and a[1] == outs[0][1] + outs[1][1] and a[2] == 2.0, (a, outs)


@pytest.mark.parametrize("B,L", SHAPES)
def test_regress_loss_non_finite_flag(B, L):
    """One pred element inf: a training step (skip flag) leaves acc and its count alone, an evaluation step adds it."""
    from sar_ssl_amd import hip
    dev = torch.device("cuda:0")
    pred, tgt = _data(B, L, 7 * B + L)
    pred[B // 2, L - 1] = np.inf
    p, t = torch.from_numpy(pred).to(dev), torch.from_numpy(tgt).to(dev)
    start = [1.5, 2.5, 3.0]
    acc = torch.tensor(start, dtype=torch.float64, device=dev)
    out, dpred = hip.regress_loss(p, t, sink=(None, acc), with_grad=True, skip_nonfinite=True)
    assert not np.isfinite(float(out[0]))
    assert acc.cpu().tolist() == start
    out = hip.regress_loss(p, t, sink=(None, acc), skip_nonfinite=False)
    a = acc.cpu().numpy()
    assert not np.isfinite(float(out[0])) and not np.isfinite(a[0]) and a[2] == 4.0
    # and a call without any sink
    out = hip.regress_loss(p, t)
    assert not np.isfinite(float(out[0]))
