"""-m gpu parity of the whole hot path (forward, CTC, backward, optimizer, BN statistics, decode)
through the C ABI against the CPU oracle on the same seeded inputs.

Tolerances (north_star): fp32 logits within 1e-3, CTC loss within 1e-3, greedy indices bit-exact;
gradients within 1e-3 of each tensor's max magnitude."""
import numpy as np
import pytest
import torch

from oracle import ops, ctc, model as M
from crnn_mi355x.engine import Engine

pytestmark = pytest.mark.gpu

FLIP_BOUND = 1e-2        # fraction of discontinuous decisions (gates, pooling arg-maxima) allowed to differ from the oracle's
GRAD_TOL_PURE = 2e-3      # device gradient vs the pure fp64 oracle's under the device's gate decisions, relative to the tensor's maximum


def masks_from_engine(eng, cfg, seed):
    """Fetch the dropout multipliers the device RNG applies and convert them to the oracle's keep-masks."""
    from gpu_util import L, P, S, ok, zeros, host
    B, T = eng.B, eng.T
    masks = {}
    h, w = cfg.Hp, cfg.Wp
    for i, (cout, pool) in enumerate(M.BLOCKS, 1):
        if pool:
            h, w = h // pool[0], w // pool[1]
        m = zeros(B * h * w * cout)
        ok(L().crnn_dropout_mask(P(m), m.numel(), M.DROP_BLOCK, seed, i, S()))
        masks[f"b{i}"] = (host(m).reshape(B, h, w, cout) > 0).astype(np.float64)
    m = zeros(T * B * cfg.tds)
    ok(L().crnn_dropout_mask(P(m), m.numel(), M.DROP_DENSE1, seed, 8, S()))
    masks["dense1"] = (host(m).reshape(T, B, cfg.tds).transpose(1, 0, 2) > 0).astype(np.float64)
    m = zeros(T * B * 2 * cfg.u)
    ok(L().crnn_dropout_mask(P(m), m.numel(), M.DROP_RNN, seed, 9, S()))
    masks["rnn"] = (host(m).reshape(T, B, 2 * cfg.u).transpose(1, 0, 2) > 0).astype(np.float64)
    return masks


def device_activation(eng, i, cin):
    """a_i = ReLU6(BatchNorm_1(d_i)) of block i as the device forms it: the pointwise kernels apply the
    BatchNorm + ReLU6 while they stage d (no `a` tensor in HBM): relu6(fma(d, scale, shift)) -- exact product + one rounding -- from the
    device's own d and BatchNorm state, the arithmetic of the staging waves."""
    f64 = lambda name: eng.ws_tensor(name).float().cpu().numpy().astype(np.float64)
    s1 = f64(f"bn1s{i}")     # (block 1 too since round 4: its outer product applies the BatchNorm to d on the way in)
    y = (f64(f"d{i}").reshape(-1, cin) * s1[2 * cin:3 * cin] + s1[3 * cin:4 * cin]).astype(np.float32).astype(np.float64)
    return np.minimum(np.maximum(y, 0), 6)     # (bf16 storage mode: the MFMA operand is this value rounded to bf16; the GATE is taken on the fp32 value, as here)


def layer_report(eng, cfg, c, B):
    """max |device - oracle| for every saved intermediate (name -> (err, scale))."""
    T = eng.T
    rep = {}

    def cmp(name, ref, tm=False):
        t = eng.ws_tensor(name).float().cpu().numpy().astype(np.float64)
        ref = np.asarray(ref, dtype=np.float64)
        if tm:
            ref = np.swapaxes(ref, 0, 1)
        t = t[:ref.size].reshape(ref.shape)
        rep[name] = (float(np.abs(t - ref).max()), float(np.abs(ref).max()))

    if eng.cfg.stn:
        for n in ("pool1", "c1", "pool2", "flat", "fc1", "theta"):
            cmp(n, c[n].reshape(B, -1))
    cmp("x0", ops.zeropad_fwd(c["xs"], 2))
    for i in range(1, 8):
        cmp(f"d{i}", c[f"d{i}"]); cmp(f"q{i}", c[f"q{i}"])
        ref = np.asarray(c[f"a{i}"], dtype=np.float64)
        a = device_activation(eng, i, ref.shape[-1]).reshape(-1)[:ref.size].reshape(ref.shape)
        rep[f"a{i}"] = (float(np.abs(a - ref).max()), float(np.abs(ref).max()))
    cmp("x7", c["conv_out"])
    cmp("dn1", c["rnn_in"], tm=True)
    cmp("h1f", c["rnn1f"][3], tm=True); cmp("h1b", c["rnn1b"][3], tm=True)
    cmp("h2", c["rnn_out"], tm=True)
    cmp("logits", c["logits"]); cmp("ypred", c["y_pred"])
    return rep


def device_cache(eng, cfg, p, x, B, c_ref, masks=None):
    """Oracle cache rebuilt from the DEVICE's forward state (fp32 -> fp64).

    ReLU6 / ReLU / hard-sigmoid gates and max-pool arg-maxima are discontinuous: with ~1e7 activations per
    step a handful sit within fp32 round-off of a threshold, and each such flip moves a per-channel gradient
    sum by a few percent.  The forward pass is checked layer by layer against the pure oracle
    (`layer_report`); the backward pass is checked against the oracle's backward evaluated on the device's own
    forward state, so both sides take identical gate decisions."""
    T = eng.T
    f64 = lambda name: eng.ws_tensor(name).float().cpu().numpy().astype(np.float64)
    c = {"x": x, "stats": {}}
    if eng.cfg.stn:
        for n in ("pool1", "c1", "pool2", "flat", "fc1", "theta"):
            c[n] = f64(n).reshape(c_ref[n].shape)
        c["c2"] = c["flat"].reshape(c_ref["c2"].shape)
    h, w, cin = cfg.Hp, cfg.Wp, 1
    prev = f64("x0").reshape(B, h, w, 1)
    c["xs"] = prev[:, 2:-2, 2:-2, :]
    for i, (cout, pool) in enumerate(M.BLOCKS, 1):
        c[f"in{i}"] = prev
        c[f"d{i}"] = f64(f"d{i}").reshape(B, h, w, cin)
        c[f"a{i}"] = device_activation(eng, i, cin).reshape(-1)[:B * h * w * cin].reshape(B, h, w, cin)
        c[f"q{i}"] = f64(f"q{i}").reshape(B, h, w, cout)
        s1, s2 = f64(f"bn1s{i}"), f64(f"bn2s{i}")
        n = B * h * w
        c["stats"][f"b{i}_bn1"] = (s1[:cin], s1[cin:2 * cin], n)
        c["stats"][f"b{i}_bn2"] = (s2[:cout], s2[cout:2 * cout], n)
        # r = relu6(fma(q, scale, shift)): exact product + one rounding, as the device's fmaf computes it
        y = (c[f"q{i}"] * s2[2 * cout:3 * cout] + s2[3 * cout:4 * cout]).astype(np.float32).astype(np.float64)
        c[f"r{i}"] = np.minimum(np.maximum(y, 0), 6)
        if pool:
            h, w = h // pool[0], w // pool[1]
        if eng.lib.crnn_block_output_fused(eng._c, i):
            # the block output exists only inside the next block's depthwise kernels (parity mode: the default schedule):
            # x = Dropout(ReLU6(BatchNorm-2(q))) as those kernels form it -- r * 1/(1-rate) in fp32, dropped elements 0
            prev = c[f"r{i}"]
            if pool:   # (round 6: a pooled block's output formed from q at the windows' arg-max = the window maximum of r)
                prev = prev.reshape(B, h, pool[0], w, pool[1], cout).max(axis=(2, 4))
            if masks is not None:
                ik = np.float32(1.0) / (np.float32(1.0) - np.float32(M.DROP_BLOCK))
                prev = (prev.astype(np.float32) * ik).astype(np.float64) * masks[f"b{i}"]
        else:
            prev = f64(f"x{i}").reshape(B, h, w, cout)
        cin = cout
    c["conv_out"] = prev
    c["feat"] = prev.reshape(B, cfg.T, cfg.feat)
    tm = lambda a, k: np.ascontiguousarray(a.reshape(T, B, k).transpose(1, 0, 2))
    c["dense1"] = tm(f64("dn1"), cfg.tds)
    c["rnn_in"] = c["dense1"]
    u, G = cfg.u, cfg.ng * cfg.u
    h2 = tm(f64("h2"), 2 * u)
    r1 = tm(f64("r1"), u)
    for name, xin, H in (("rnn1f", c["rnn_in"], tm(f64("h1f"), u)), ("rnn1b", c["rnn_in"], tm(f64("h1b"), u)),
                         ("rnn2f", r1, h2[..., :u]), ("rnn2b", r1, h2[..., u:])):
        l, d = name[3], name[4]
        if cfg.gru:
            c[name] = (xin, p[name + "_w"], p[name + "_u"], H, tm(f64(f"gt{l}{d}"), G), d == "b")
        else:
            c[name] = (xin, p[name + "_w"], p[name + "_u"], H, tm(f64(f"cs{l}{d}"), u), tm(f64(f"gt{l}{d}"), G), d == "b")
    c["rnn_out"] = h2
    c["dense2_in"] = tm(f64("r2d"), 2 * u)
    c["y_pred"] = f64("ypred").reshape(B, T, cfg.num_classes)
    return c


def hybrid_cache(cfg, c, cdev, stn, masks=None):
    """The PURE fp64 oracle cache with the device's value substituted wherever a discontinuous decision differs between the two
    forwards: ReLU6 gates of a_i / r_i (0 < y < 6), the first-maximum position of every pooling window (whole window substituted),
    dense1's and the localisation net's ReLU (y > 0), the hard-sigmoid gates of the recurrent cells (0 < a < 1).  The oracle's
    backward on this cache takes the DEVICE's decisions everywhere but keeps the oracle's own values elsewhere: the device's
    gradients must agree with it to the parity tolerance -- no flip noise left to hide a backward bug behind.
    -> (cache, number of differing decisions, number of decisions)"""
    h = dict(c)
    flips, total = 0, 0
    by_kind = {}

    def count(kind, n):
        by_kind[kind] = by_kind.get(kind, 0) + int(n)

    def gate(ref, dev, lo, hi, where=None, kind="relu6"):
        nonlocal flips, total
        ref = np.array(ref, dtype=np.float64, copy=True)
        dev = np.asarray(dev, dtype=np.float64).reshape(ref.shape)
        dref = (ref > lo) if hi is None else ((ref > lo) & (ref < hi))
        ddev = (dev > lo) if hi is None else ((dev > lo) & (dev < hi))
        diff = dref != ddev
        if where is not None:
            diff &= np.asarray(where).reshape(ref.shape) > 0
        flips += int(diff.sum()); total += ref.size; count(kind, diff.sum())
        ref[diff] = dev[diff]
        return ref

    def windows(ref, dev, ph, pw):
        """substitute every pooling window whose first-maximum position differs"""
        nonlocal flips, total
        B, H, W, C = ref.shape
        Ho, Wo = H // ph, W // pw
        view = lambda a: a[:, :Ho * ph, :Wo * pw, :].reshape(B, Ho, ph, Wo, pw, C).transpose(0, 1, 3, 2, 4, 5).reshape(B, Ho, Wo, ph * pw, C)
        rv, dv = view(ref).copy(), view(np.asarray(dev, dtype=np.float64).reshape(ref.shape))
        diff = rv.argmax(axis=3) != dv.argmax(axis=3)
        flips += int(diff.sum()); total += diff.size; count("pool", diff.sum())
        sel = np.broadcast_to(diff[:, :, :, None, :], rv.shape)
        rv[sel] = dv[sel]
        out = np.array(ref, copy=True)
        out[:, :Ho * ph, :Wo * pw, :] = rv.reshape(B, Ho, Wo, ph, pw, C).transpose(0, 1, 3, 2, 4, 5).reshape(B, Ho * ph, Wo * pw, C)
        return out

    for i, (cout, pool) in enumerate(M.BLOCKS, 1):
        h[f"a{i}"] = gate(c[f"a{i}"], cdev[f"a{i}"], 0.0, 6.0)
        r = gate(c[f"r{i}"], cdev[f"r{i}"], 0.0, 6.0)
        if pool:
            r = windows(r, cdev[f"r{i}"], *pool)
        h[f"r{i}"] = r
    # (the device keeps dense1 with its dropout applied: entries the mask drops carry no gradient and are not decisions)
    h["dense1"] = gate(c["dense1"], cdev["dense1"], 0.0, None, where=(masks or {}).get("dense1"), kind="relu")
    gi = 4 if cfg.gru else 5          # position of the activated gates in the cell cache tuple
    for name in ("rnn1f", "rnn1b", "rnn2f", "rnn2b"):
        t = list(c[name])
        t[gi] = gate(t[gi], cdev[name][gi], 0.0, 1.0, kind="hard_sigmoid")
        h[name] = tuple(t)
    if stn:
        h["fc1"] = gate(c["fc1"], cdev["fc1"], 0.0, None, kind="relu")
        h["c1"] = windows(np.asarray(c["c1"], dtype=np.float64), cdev["c1"], 2, 2)
    return h, flips, total, by_kind


class Case(tuple):
    """run_case's 13 results + .hybrid = (gradients of the oracle's backward on hybrid_cache, differing decisions, decisions)"""
    hybrid = None


def hot_batchnorm(cfg, p, seed=5):
    """The conv stack's BatchNorm layers at gamma = 2 (1 + 0.3 U(-1, 1)), beta = 3 + 0.6 U(-1, 1): with batch statistics every pre-activation is about
    N(3, 2^2), so 6-7 % of each a_i / r_i sit at the ReLU6 ceiling and as many at the floor (randomize_params leaves about N(0, 1): half at the floor, 1e-4 to
    none at the ceiling).  Drawn from RandomState(seed): blocks 1..7, bn1 then bn2, gamma then beta."""
    rs = np.random.RandomState(seed)
    for i in range(1, len(M.BLOCKS) + 1):
        for j in (1, 2):
            g, b = f"b{i}_bn{j}_g", f"b{i}_bn{j}_b"
            p[g] = (2 * (1 + 0.3 * rs.uniform(-1, 1, p[g].shape))).astype(p[g].dtype)
            p[b] = (3 + 0.6 * rs.uniform(-1, 1, p[b].shape)).astype(p[b].dtype)
    return p


def assert_hot_coverage(c, tag):
    """Every ReLU6 of the oracle's forward decides at both ends: at least 3 % of each a_i and r_i at 6 and at least 3 % at 0."""
    for i in range(1, len(M.BLOCKS) + 1):
        for name in (f"a{i}", f"r{i}"):
            t = np.asarray(c[name])
            hi, lo = float((t == 6).mean()), float((t == 0).mean())
            assert hi >= 0.03 and lo >= 0.03, f"{tag}: {name} has {hi:.3f} of its elements at the ceiling and {lo:.3f} at the floor"


def run_case(B, imgh, imgw, u, tds, max_len, stn, dropout, seed=3, num_classes=38, gru=False, variable_width=False, flags=None, params_hook=None):
    cfg = M.Config(imgh=imgh, imgw=imgw, num_classes=num_classes, max_len=max_len, time_dense_size=tds, n_units=u, gru=gru)
    p, bn = M.init_params(cfg, seed=7, dtype=np.float64)
    p = M.randomize_params(cfg, p)
    if params_hook is not None:
        p = params_hook(cfg, p)
    x, lab, il, ll = M.synthetic_batch(cfg, B, seed=1, dtype=np.float64, variable_width=variable_width)
    eng = Engine(B, imgh, imgw, num_classes, max_len, tds, u, gru=gru, stn=stn, dropout=dropout, flags=flags)
    eng.set_params(p, bn)
    masks = masks_from_engine(eng, cfg, seed) if dropout else None
    # ---- device
    yd = eng.forward(x.astype(np.float32), train=True, seed=seed).cpu().numpy()
    loss_d = eng.backward(lab, il, ll, seed=seed).cpu().numpy()
    gd = eng.get_grads()
    # ---- pure oracle (fp64): forward parity, loss parity, and a flip-tolerant look at the gradients
    loss, loss_b, g, c = M.loss_and_grads(cfg, p, bn, x, lab, il, ll, masks=masks, stn=stn)
    rep = layer_report(eng, cfg, c, B)
    # ---- oracle backward on the device's forward state: exact gradient parity
    cdev = device_cache(eng, cfg, p, x, B, c, masks)
    _, gy = ctc.ctc_loss_and_grad(cdev["y_pred"], lab, il, ll)
    if masks is not None:   # dense1 holds the dropped activation on the device: its mask is already applied
        masks_dev = dict(masks)
    else:
        masks_dev = None
    gdev = M.backward(cfg, p, cdev, gy / B, masks=masks_dev, stn=stn)
    # ---- pure oracle values, the device's gate decisions (hybrid_cache): the pure-oracle gradient check without flip noise
    ch, flips, decisions, by_kind = hybrid_cache(cfg, c, cdev, stn, masks)
    _, gy_ref = ctc.ctc_loss_and_grad(c["y_pred"], lab, il, ll)
    ghyb = M.backward(cfg, p, ch, gy_ref / B, masks=masks, stn=stn)
    res = Case((cfg, eng, p, bn, (x, lab, il, ll), yd, loss_d, gd, c, loss_b, g, rep, gdev))
    res.hybrid = (ghyb, flips, decisions, by_kind)
    return res


def check_case(res, tag):
    cfg, eng, p, bn, batch, yd, loss_d, gd, c, loss_b, g, rep, gdev = res
    bad = {k: v for k, v in rep.items() if v[0] > 1e-3 * max(1.0, v[1])}
    assert not bad, f"{tag}: intermediates off: {bad}"
    assert np.abs(c["logits"] - eng.ws_tensor("logits").float().cpu().numpy().reshape(c["logits"].shape)).max() < 1e-3
    assert np.abs(yd - c["y_pred"]).max() < 1e-4
    assert np.all(np.abs(loss_d - loss_b) < 1e-3 + 1e-5 * np.abs(loss_b)), (loss_d, loss_b)
    worst = {}
    for k in p:
        scale = max(np.abs(gdev[k]).max(), 1e-6)
        if "_bn" in k:
            # d(gamma) and d(beta) of one BatchNorm layer are sums over the same B*H*W terms; with few channels (block 1 has ONE) a
            # sum that cancels to a small value would otherwise be judged against itself instead of against the size of its terms
            # (seen on variable-width text: d(beta) = -0.68 next to d(gamma) = 7.3, fp32 round-off of the 29 k-term sum 4e-3)
            scale = max(scale, np.abs(gdev[k[:-1] + "g"]).max(), np.abs(gdev[k[:-1] + "b"]).max())
        err = np.abs(gd[k] - gdev[k]).max()
        if err > 1e-3 * scale + 1e-7:
            worst[k] = (err / scale)
    assert not worst, f"{tag}: gradient mismatch vs oracle-on-device-state {worst}"
    # pure fp64 oracle.  The two forwards take a handful of different discontinuous decisions (ReLU6 / ReLU / hard-sigmoid gates,
    # pooling arg-maxima: activations within fp32 round-off of a threshold): their number is bounded, and with the device's decisions
    # substituted into the oracle's own fp64 cache (hybrid_cache) every gradient must agree to the parity tolerance
    ghyb, flips, decisions, by_kind = res.hybrid
    print(f"[{tag}] discontinuous decisions differing between the fp32 device forward and the fp64 oracle: {flips} of {decisions} {by_kind}")
    off = {}
    for k in p:
        scale = max(np.abs(ghyb[k]).max(), 1e-6)
        if "_bn" in k:
            scale = max(scale, np.abs(ghyb[k[:-1] + "g"]).max(), np.abs(ghyb[k[:-1] + "b"]).max())
        err = np.abs(gd[k] - ghyb[k]).max()
        if err > GRAD_TOL_PURE * scale + 1e-7:
            off[k] = err / scale
    print(f"[{tag}] worst gradient error vs the pure oracle under the device's decisions: "
          f"{max((np.abs(gd[k] - ghyb[k]).max() / max(np.abs(ghyb[k]).max(), 1e-6)) for k in p):.3e}")
    assert not off, f"{tag}: gradients differ from the pure oracle evaluated under the device's gate decisions {off}"
    assert flips <= FLIP_BOUND * decisions, f"{tag}: {flips} of {decisions} gate / arg-max decisions differ from the oracle's {by_kind}"


def test_small_model_no_dropout():
    check_case(run_case(B=5, imgh=40, imgw=32, u=64, tds=32, max_len=6, stn=True, dropout=False), "small")


def test_small_model_with_device_dropout_masks():
    check_case(run_case(B=4, imgh=40, imgw=32, u=64, tds=32, max_len=6, stn=True, dropout=True), "small+dropout")


def test_small_gru_model_with_dropout():
    """The GRU variant is what the reference's train.py actually builds."""
    check_case(run_case(B=4, imgh=40, imgw=32, u=64, tds=32, max_len=6, stn=True, dropout=True, gru=True), "small-gru")


def test_config1_shape_gru_model():
    check_case(run_case(B=4, imgh=100, imgw=32, u=256, tds=128, max_len=23, stn=True, dropout=False, gru=True), "config1-gru")


_BS64 = {}


def _bs64_case():
    """BASELINE.json's metric names "100x32 bs64": the full-width model (n_units 256, time_dense_size 128, max_len 23, LSTM, spatial transformer)
    in TRAINING mode (batch statistics, dropout on, gradients) at batch 64, parity mode with its default flags, against the fp64 oracle.  The oracle
    pass (forward + three backwards over 64 images) is the expensive part (~1-2 min of host time), so it runs once per session and the
    strict-backward test below re-uses its references: both flag sets take the same forward bit for bit, hence the same device state, the same
    gate decisions and the same oracle gradients."""
    if "res" not in _BS64:
        _BS64["res"] = run_case(B=64, imgh=100, imgw=32, u=256, tds=128, max_len=23, stn=True, dropout=True, seed=11)
    return _BS64["res"]


def test_bs64_training_step_matches_the_oracle_default_flags():
    """(utils.py:58-103 at the metric's literal batch; the backward GEMMs carry two bf16 planes per operand -- the parity mode's default.)"""
    check_case(_bs64_case(), "bs64")


def test_bs64_training_step_matches_the_oracle_three_plane_backward():
    """The same batch-64 training step under CRNN_FLAG_THREE_PLANE_BACKWARD (every backward GEMM with fp32-accurate products): the forward is the
    default flags' bit for bit (asserted), so the oracle references of the default-flags case apply unchanged; every gradient tensor within the
    same tolerances."""
    from crnn_mi355x import native
    res = _bs64_case()
    cfg, eng0, p, bn, (x, lab, il, ll), yd, loss_d, gd0, c, loss_b, g, rep, gdev = res
    eng = Engine(64, 100, 32, 38, 23, 128, 256, stn=True, dropout=True, flags=native.FLAG_THREE_PLANE_BACKWARD)
    eng.set_params(p, bn)
    y = eng.forward(x.astype(np.float32), train=True, seed=11).cpu().numpy()
    loss = eng.backward(lab, il, ll, seed=11).cpu().numpy()
    assert np.array_equal(y, yd) and np.array_equal(loss, loss_d), "the backward's product precision changed the forward"
    for name in ("q3", "q7", "dn1", "h2"):
        assert torch.equal(eng.ws_tensor(name), eng0.ws_tensor(name)), name
    strict = Case((cfg, eng, p, bn, (x, lab, il, ll), y, loss, eng.get_grads(), c, loss_b, g, rep, gdev))
    strict.hybrid = res.hybrid
    check_case(strict, "bs64 three-plane backward")
    # and the two backward precisions against each other at this batch: within 1e-4 of each tensor's largest element
    gs = strict[7]
    worst = max(float(np.abs(gs[k] - gd0[k]).max() / max(np.abs(gs[k]).max(), 1e-12)) for k in gs)
    print("bs64: two-plane vs three-plane backward, worst tensor %.3g of its maximum" % worst)
    assert worst < 1e-3, worst


# bf16s (the throughput mode) gradient bounds, measured on MI355X in round 6 (visit r06g) and asserted at twice the measured worst tensor:
#   * "own state": the oracle's fp64 backward evaluated on the DEVICE's forward state (bf16 tensors as stored, BatchNorm statistics of the values as stored,
#     the device's dropout decisions) -- what is left is the backward's own arithmetic: bf16 products, bf16 gradient tensors in the conv stack;
#   * "hybrid": the pure fp64 oracle's values with the device's discontinuous decisions substituted (hybrid_cache) -- forward + backward error together.
# Measured worst tensors (visit r06h; own state / hybrid): small 1.6e-2 / 8.2e-2, config-1 shape 3.0e-2 / 8.0e-2, batch 64 9.9e-2 (b1_bn2_b: 240 k cancelling terms
# per channel behind bf16 gradient tensors) / 1.7e-1 (stn_d2_b); differing decisions 4.1e-3 of all, nine tenths of them ReLU6 gates of bf16-rounded values.
BF16S_OWN_STATE_TOL = {"small": 3.5e-2, "config1": 6e-2, "bs64": 2e-1}
BF16S_HYBRID_TOL = {"small": 1.7e-1, "config1": 1.7e-1, "bs64": 3.5e-1}
# ... and the tensors from dense2 down to block 2's pointwise kernel individually against the backward on the device's own state (2 x the largest measured)
BF16S_TOP = {"dense2_w": 5e-5, "dense2_b": 5e-5, "rnn2f_w": 2e-3, "rnn2b_u": 2e-3, "rnn1f_w": 3e-3, "dense1_w": 6e-3, "b7_pw": 1e-2, "b6_pw": 1.3e-2, "b5_pw": 3e-2,
             "b4_pw": 3e-2, "b3_pw": 3e-2, "b2_pw": 6.5e-2}
# The hot regime (hot_batchnorm: 6-7 % of every ReLU6 at each end) asserts none of the figures above.  Its bound is the oracle's own: D(k), the distance
# between the fp64 backward with ReLU6's gradient and with ReLU's (ceiling term removed), both on the device's forward state; the device must lie within
# D(k) / 4 of the former (_ceiling_bound).
# Measured in the hot regime on MI355X (own state, each tensor relative to its own largest element; 42 conv-stack tensors, all with D >= 0.2):
#   small         worst error / D 2.3e-2 (b1_bn1_g: error 2.3e-1 of a one-element tensor, D 70); next worst error 2.1e-2 (b1_dw, D 1.5); smallest D 0.43 (b7_bn2_b)
#   small, tile   worst error / D 3.5e-2; worst error 2.3e-1 (b1_bn1_g again); smallest D 0.43
#   config-1      worst error / D 2.0e-2; worst error 4.0e-2 (b1_bn1_b, D 3.0); smallest D 0.20 (b7_bn2_b), median about 1.0
# With the clamps of the bf16 staging kernels turned into ReLU (a scratch build) the pointwise weight gradients of blocks 4-7 sit at 0.26 - 0.32 against D 0.36 - 1.0.
# Parity mode, hot (check_case, its own constants): worst gradient error against the pure oracle under the device's decisions 6.4e-5 (small), 1.4e-4 (small +
# dropout), 1.2e-4 (config-1, either backward); differing decisions 1.3e-4 / 6.4e-5 / 3.0e-4 of all, ReLU6 gates among them 11 / 13 / 29 (cold small: 75 / 67).
HOT_SEED = 6              # hot_batchnorm's default seed 5 leaves block 1's single BatchNorm-1 channel with 2.8 % of a1 at the floor; seed 6 gives >= 5.6 % everywhere
CEILING_MIN_D = 0.2       # conv-stack tensors the ceiling moves by less than this (of their maximum) are not judged; at most a quarter of them
CEILING_FACTOR = 4        # the device at least four times nearer to ReLU6's gradient than to ReLU's


def _ceiling_bound(tag, cfg, p, cdev, g_ypred, masks, gd, gdev):
    """gdev: the oracle's backward on the device's forward state.  The same backward with the ceiling term of ReLU6's gradient removed (gy * (y > 0))
    gives D(k) = max |difference| / max |gdev[k]| for every conv-stack tensor; where D(k) >= CEILING_MIN_D the device's gradient must be within
    D(k) / CEILING_FACTOR of gdev[k].  -> {k: (device error, D(k))}"""
    keep = ops.relu6_bwd_from_out
    try:
        ops.relu6_bwd_from_out = lambda y, gy: gy * (y > 0)
        grelu = M.backward(cfg, p, cdev, g_ypred, masks=masks, stn=True)
    finally:
        ops.relu6_bwd_from_out = keep
    out = {}
    for k in p:
        if k[0] == "b" and k[1].isdigit() and any(s in k for s in ("_dw", "_pw", "_bn")):
            top = max(np.abs(gdev[k]).max(), 1e-30)
            out[k] = (float(np.abs(gd[k] - gdev[k]).max() / top), float(np.abs(grelu[k] - gdev[k]).max() / top))
    assert len(out) == 6 * len(M.BLOCKS)
    for k, (e, d) in out.items():
        print(f"[{tag} hot] {k}: device error {e:.3e} of the maximum, D = {d:.3e}")
    judged = {k: v for k, v in out.items() if v[1] >= CEILING_MIN_D}
    print(f"[{tag} hot] worst device error {max(v[0] for v in out.values()):.3e}; worst error / D {max(e / d for e, d in judged.values()):.3e}; "
          f"smallest D {min(v[1] for v in out.values()):.3e}; judged {len(judged)} of {len(out)}")
    assert 4 * (len(out) - len(judged)) <= len(out), f"{tag}: the ceiling moves too few tensors: {sorted(set(out) - set(judged))}"
    bad = {k: v for k, v in judged.items() if v[0] > v[1] / CEILING_FACTOR}
    assert not bad, f"{tag}: the device's gradient is not four times nearer to ReLU6's than to ReLU's (error, D): {bad}"
    return out


def _bf16s_gradient_case(tag, B, imgh, imgw, u, tds, max_len, seed, ref=None, flags=None, params_hook=None):
    """One bf16s training step (dropout on, device masks) against the fp64 oracle's backward under the device's own decisions.  ref: a parity-mode Case of the
    same configuration, inputs and seed (re-uses its parameters, batch and pure-oracle cache)."""
    if ref is None:
        cfg = M.Config(imgh=imgh, imgw=imgw, max_len=max_len, time_dense_size=tds, n_units=u)
        p, bn = M.init_params(cfg, seed=7, dtype=np.float64)
        p = M.randomize_params(cfg, p)
        if params_hook is not None:
            p = params_hook(cfg, p)
        x, lab, il, ll = M.synthetic_batch(cfg, B, seed=1, dtype=np.float64)
        c = None
    else:
        cfg, _, p, bn, (x, lab, il, ll), c = ref[0], ref[1], ref[2], ref[3], ref[4], ref[8]
    eng = Engine(B, imgh, imgw, 38, max_len, tds, u, stn=True, dropout=True, precision="bf16s", flags=flags)
    eng.set_params(p, bn)
    masks = masks_from_engine(eng, cfg, seed)
    if c is None:
        _, _, _, c = M.loss_and_grads(cfg, p, bn, x, lab, il, ll, masks=masks, stn=True)
    yd = eng.forward(x.astype(np.float32), train=True, seed=seed).cpu().numpy()
    loss_d = eng.backward(lab, il, ll, seed=seed).cpu().numpy()
    gd = eng.get_grads()
    assert all(np.isfinite(v).all() for v in gd.values())
    cdev = device_cache(eng, cfg, p, x, B, c, masks)
    _, gy = ctc.ctc_loss_and_grad(cdev["y_pred"], lab, il, ll)
    gdev = M.backward(cfg, p, cdev, gy / B, masks=dict(masks), stn=True)
    ch, flips, decisions, by_kind = hybrid_cache(cfg, c, cdev, True, masks)
    _, gy_ref = ctc.ctc_loss_and_grad(c["y_pred"], lab, il, ll)
    ghyb = M.backward(cfg, p, ch, gy_ref / B, masks=masks, stn=True)

    def errs(ref_g):
        out = {}
        for k in p:
            scale = max(np.abs(ref_g[k]).max(), 1e-6)
            if "_bn" in k:
                scale = max(scale, np.abs(ref_g[k[:-1] + "g"]).max(), np.abs(ref_g[k[:-1] + "b"]).max())
            out[k] = float(np.abs(gd[k] - ref_g[k]).max() / scale)
        return out
    e_own, e_hyb = errs(gdev), errs(ghyb)
    w_own, w_hyb = max(e_own, key=e_own.get), max(e_hyb, key=e_hyb.get)
    print(f"[bf16s {tag}] decisions differing from the fp64 oracle's: {flips} of {decisions} ({flips / decisions:.2e}) {by_kind}")
    print(f"[bf16s {tag}] gradients vs the oracle backward on the device's own state: worst {w_own} {e_own[w_own]:.3e} of its maximum; "
          + " ".join(f"{k}:{e_own[k]:.1e}" for k in BF16S_TOP))
    print(f"[bf16s {tag}] gradients vs the pure oracle under the device's decisions:   worst {w_hyb} {e_hyb[w_hyb]:.3e} of its maximum; "
          + " ".join(f"{k}:{e_hyb[k]:.1e}" for k in BF16S_TOP))
    if params_hook is not None:       # the hot regime: the bounds below were measured in the cold one and are not re-used; the bound comes from the oracle alone
        assert_hot_coverage(c, f"bf16s {tag}")
        return _ceiling_bound(f"bf16s {tag}", cfg, p, cdev, gy / B, dict(masks), gd, gdev)
    tile = tag.endswith("-tile")      # the tile schedule runs dense2's backward and the recurrent projections' gradients as bf16 tile GEMMs (measured 6e-4 / 3.5e-3)
    tag = tag.split("-")[0]
    cap = lambda k: BF16S_TOP.get(k, 1.0) if not tile else max(2 * BF16S_TOP.get(k, 1.0), 1.5e-3)
    bad = {k: v for k, v in e_own.items() if v > min(BF16S_OWN_STATE_TOL[tag], cap(k))}
    assert not bad, f"bf16s {tag}: backward differs from the oracle's on the device's own forward state: {bad}"
    bad = {k: v for k, v in e_hyb.items() if v > BF16S_HYBRID_TOL[tag]}
    assert not bad, f"bf16s {tag}: gradients differ from the pure oracle's under the device's decisions: {bad}"
    return e_own, e_hyb


@pytest.mark.parametrize("tag", ["small", "small-tile", "config1", "config1-tile", "bs64"])
def test_bf16s_training_step_gradients_under_the_device_decisions(tag):
    """The mode that is benchmarked (bf16 products, bf16 conv-stack tensors) gets the parity mode's gradient check: the fp64 oracle's backward under the
    device's own gate / arg-max / dropout decisions, every gradient tensor bounded relative to its largest element -- at a small shape, at the config-1
    shape and at the metric's literal batch 64, full width (utils.py:58-103); the default schedule (weights-resident / streaming kernels) and, at the two
    small shapes, the tile schedule (CRNN_FLAG_GEMM_TILE_KERNELS).  A wrong scale factor, a dropped term or a transposed operand anywhere in the bf16
    backward moves a tensor by O(1) of its maximum; bf16 round-off moves it by the figures in the tables above."""
    from crnn_mi355x import native
    flags = native.FLAG_GEMM_TILE_KERNELS if tag.endswith("-tile") else None
    if tag.startswith("small"):
        _bf16s_gradient_case(tag, B=4, imgh=40, imgw=32, u=128, tds=64, max_len=6, seed=3, flags=flags)
    elif tag.startswith("config1"):
        _bf16s_gradient_case(tag, B=4, imgh=100, imgw=32, u=256, tds=128, max_len=23, seed=3, flags=flags)
    else:
        _bf16s_gradient_case(tag, B=64, imgh=100, imgw=32, u=256, tds=128, max_len=23, seed=11, ref=_bs64_case())


# ---- the hot regime: every ReLU6 of the conv stack decides at both ends (hot_batchnorm), same checks and constants as the cold cases
def _hot_params(cfg, p):
    return hot_batchnorm(cfg, p, seed=HOT_SEED)


def _hot_case(tag, **kw):
    res = run_case(params_hook=_hot_params, **kw)
    assert_hot_coverage(res[8], tag)
    return res


@pytest.mark.parametrize("dropout", [False, True])
def test_hot_small_model_matches_the_oracle(dropout):
    """check_case unchanged on the small LSTM model with 6-7 % of every a_i / r_i at the ReLU6 ceiling and as many at the floor: a kernel that gated with
    ReLU's mask at any backward site, or clamped only at 0 at any forward site, moves its tensors by O(0.1 - 1) of their maximum here."""
    tag = "hot small+dropout" if dropout else "hot small"
    check_case(_hot_case(tag, B=5, imgh=40, imgw=32, u=64, tds=32, max_len=6, stn=True, dropout=dropout), tag)


_HOT_CONFIG1 = {}


def _hot_config1_case():
    """The config-1 shape (the one at which the engine picks its resident and row-stream schedules) at batch 4, dropout on, hot: one oracle pass for both flag sets."""
    if "res" not in _HOT_CONFIG1:
        _HOT_CONFIG1["res"] = _hot_case("hot config1", B=4, imgh=100, imgw=32, u=256, tds=128, max_len=23, stn=True, dropout=True)
    return _HOT_CONFIG1["res"]


def test_hot_config1_shape_matches_the_oracle_default_flags():
    check_case(_hot_config1_case(), "hot config1")


def test_hot_config1_shape_matches_the_oracle_three_plane_backward():
    """The same step under CRNN_FLAG_THREE_PLANE_BACKWARD: the forward is the default flags' bit for bit (asserted), so the oracle references apply unchanged."""
    from crnn_mi355x import native
    res = _hot_config1_case()
    cfg, eng0, p, bn, (x, lab, il, ll), yd, loss_d, gd0, c, loss_b, g, rep, gdev = res
    eng = Engine(4, 100, 32, 38, 23, 128, 256, stn=True, dropout=True, flags=native.FLAG_THREE_PLANE_BACKWARD)
    eng.set_params(p, bn)
    y = eng.forward(x.astype(np.float32), train=True, seed=3).cpu().numpy()
    loss = eng.backward(lab, il, ll, seed=3).cpu().numpy()
    assert np.array_equal(y, yd) and np.array_equal(loss, loss_d), "the backward's product precision changed the forward"
    for name in ("q3", "q7", "dn1", "h2"):
        assert torch.equal(eng.ws_tensor(name), eng0.ws_tensor(name)), name
    strict = Case((cfg, eng, p, bn, (x, lab, il, ll), y, loss, eng.get_grads(), c, loss_b, g, rep, gdev))
    strict.hybrid = res.hybrid
    check_case(strict, "hot config1 three-plane backward")


@pytest.mark.parametrize("tag", ["small", "small-tile", "config1"])
def test_hot_bf16s_training_step_is_nearer_to_relu6_than_to_relu(tag):
    """The benchmarked mode in the hot regime, both schedules at the small shape: every conv-stack gradient tensor the ceiling moves by at least 0.2 of its
    maximum lies within a quarter of that distance of the oracle's ReLU6 backward on the device's own forward state (_ceiling_bound)."""
    from crnn_mi355x import native
    flags = native.FLAG_GEMM_TILE_KERNELS if tag.endswith("-tile") else None
    if tag.startswith("small"):
        _bf16s_gradient_case(tag, B=4, imgh=40, imgw=32, u=128, tds=64, max_len=6, seed=3, flags=flags, params_hook=_hot_params)
    else:
        _bf16s_gradient_case(tag, B=4, imgh=100, imgw=32, u=256, tds=128, max_len=23, seed=3, flags=flags, params_hook=_hot_params)


def test_odd_shape_model_wide_image_small_alphabet():
    """A shape none of the reference's configurations use: 60 x 48 images (maps 64x52 -> 32x26 -> 32x13, so the depthwise
    tiles, the pooled BN backward and the localisation net all see odd extents), 20 classes, max_len 10, 128 units
    (bf16-capable width), dropout on."""
    res = run_case(B=5, imgh=60, imgw=48, u=128, tds=64, max_len=10, stn=True, dropout=True, num_classes=20)
    check_case(res, "odd-shape")
    # the throughput mode at the same shape: close to the fp32 engine's posteriors, finite deterministic gradients
    cfg, eng32, p, bn, (x, lab, il, ll), yd = res[0], res[1], res[2], res[3], res[4], res[5]
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)      # round 5: image width 48 takes the row-stream depthwise kernels -- no half-rate fallback, no warning
        Engine._warned_shapes.discard((60, 48))
        eng = Engine(5, 60, 48, 20, 10, 64, 128, stn=True, dropout=True, precision="bf16s")
    h, w, cin = 64, 52, 1
    for i, (co, ph, pw) in enumerate(((64, 1, 1), (128, 1, 1), (256, 2, 2), (256, 1, 1), (512, 1, 2), (512, 1, 1), (512, 1, 1)), 1):
        if i >= 2:
            assert eng.lib.crnn_dwconv_fwd_stream_supported(5, h, w, cin) == 0 and eng.lib.crnn_dwconv_bwd_stream_supported(5, h, w, cin) == 0, (i, h, w, cin)
        h, w, cin = h // ph, w // pw, co
    eng.set_params(p, bn)
    y16 = eng.forward(x.astype(np.float32), train=True, seed=3).cpu().numpy()
    assert np.abs(y16 - yd).max() < 5e-2
    l1 = eng.backward(lab, il, ll, seed=3).clone(); g1 = eng.grads.clone()
    eng.forward(x.astype(np.float32), train=True, seed=3); l2 = eng.backward(lab, il, ll, seed=3)
    assert torch.equal(l1, l2) and torch.equal(g1, eng.grads) and torch.isfinite(g1).all()


def test_width64_model_matches_the_oracle_on_the_row_stream_kernels():
    """Image width 64 (maps 44 x 68 -> 22 x 34 -> 22 x 17; round 5: its depthwise stages run the row-stream kernels -- step rows of 544 columns, bf16 / fp32 rows
    cut into channel ranges from block 3 on): the parity-mode train step against the oracle like every other shape, and the throughput mode close to it."""
    res = run_case(B=3, imgh=40, imgw=64, u=128, tds=32, max_len=6, stn=True, dropout=True)
    check_case(res, "width-64")
    cfg, eng32, p, bn, (x, lab, il, ll), yd = res[0], res[1], res[2], res[3], res[4], res[5]
    h, w, cin = 44, 68, 1
    for i, (co, ph, pw) in enumerate(((64, 1, 1), (128, 1, 1), (256, 2, 2), (256, 1, 1), (512, 1, 2), (512, 1, 1), (512, 1, 1)), 1):
        if i >= 2:
            for dt in (0, 1):
                assert eng32.lib.crnn_dwconv_fwd_stream_supported_ex(3, h, w, cin, dt) == 0 and eng32.lib.crnn_dwconv_bwd_stream_supported_ex(3, h, w, cin, dt) == 0, (i, h, w, cin, dt)
        h, w, cin = h // ph, w // pw, co
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        Engine._warned_shapes.discard((40, 64))
        eng = Engine(3, 40, 64, 38, 6, 32, 128, stn=True, dropout=True, precision="bf16s")
    eng.set_params(p, bn)
    y16 = eng.forward(x.astype(np.float32), train=True, seed=3).cpu().numpy()
    assert np.abs(y16 - yd).max() < 5e-2
    l1 = eng.backward(lab, il, ll, seed=3).clone(); g1 = eng.grads.clone()
    eng.forward(x.astype(np.float32), train=True, seed=3); l2 = eng.backward(lab, il, ll, seed=3)
    assert torch.equal(l1, l2) and torch.equal(g1, eng.grads) and torch.isfinite(g1).all()


@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16s"])
@pytest.mark.parametrize("shape", [(5, 60, 48, 20, 10, 64, 128), (3, 40, 32, 38, 6, 32, 64), (4, 100, 32, 38, 23, 128, 256), (3, 40, 64, 38, 6, 32, 128)])
def test_step_does_not_depend_on_workspace_contents(precision, shape):
    """Every workspace region a kernel reads must have been written by this step: a train step on a NaN-filled workspace
    gives bit-identical posteriors, losses and gradients to one on a zero-filled workspace (catches 0 * garbage in tile
    tails, split-K scratch and halo reads)."""
    B, imgh, imgw, ncls, max_len, tds, u = shape
    if precision != "fp32" and u % 128:
        pytest.skip("bf16 recurrent products need n_units % 128 == 0")
    cfg = M.Config(imgh=imgh, imgw=imgw, max_len=max_len, time_dense_size=tds, n_units=u, num_classes=ncls)
    p, bn = M.init_params(cfg, seed=5, dtype=np.float64)
    p = M.randomize_params(cfg, p)
    x, lab, il, ll = M.synthetic_batch(cfg, B, seed=2, dtype=np.float64)
    eng = Engine(B, imgh, imgw, ncls, max_len, tds, u, stn=True, dropout=True, precision=precision)
    eng.set_params(p, bn)
    runs = []
    for fill in (0.0, float("nan"), 0.0):
        eng.ws.fill_(fill); eng.grads.fill_(fill)
        y = eng.forward(x.astype(np.float32), train=True, seed=9).clone()
        loss = eng.backward(lab, il, ll, seed=9).clone()
        runs.append((y, loss, eng.grads.clone()))
        yi = eng.forward(x.astype(np.float32), train=False).clone()
        runs[-1] += (yi,)
    for r in runs:
        assert all(bool(torch.isfinite(t).all()) for t in r)
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
    for a, b in zip(runs[0], runs[2]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("precision", ["fp32", "bf16s"])
def test_block1_folded_batchnorm_kernels_equal_the_standalone_kernels(precision):
    """Block 1's single-channel stage with BatchNorm-1 folded into the neighbouring kernels (default, round 4) against its stand-alone kernels
    (CRNN_FLAG_BLOCK1_KERNELS): the same arithmetic with BatchNorm-1's forward and backward statistics summed in another order -- posteriors, loss and
    gradients agree to that round-off (re-rounded through bf16 tensors in the throughput mode)."""
    from crnn_mi355x import native
    B, imgh, imgw, ncls, max_len, tds, u = 6, 100, 32, 38, 23, 128, 256
    cfg = M.Config(imgh=imgh, imgw=imgw, max_len=max_len, time_dense_size=tds, n_units=u, num_classes=ncls)
    p, bn = M.init_params(cfg, seed=6, dtype=np.float64)
    p = M.randomize_params(cfg, p)
    x, lab, il, ll = M.synthetic_batch(cfg, B, seed=4, dtype=np.float64)
    out = {}
    for flags in (0, native.FLAG_BLOCK1_KERNELS):
        eng = Engine(B, imgh, imgw, ncls, max_len, tds, u, stn=True, dropout=True, precision=precision, flags=flags)
        eng.set_params(p, bn)
        eng.ws.fill_(float("nan")); eng.grads.zero_()
        y = eng.forward(x.astype(np.float32), train=True, seed=5).clone()
        loss = eng.backward(lab, il, ll, seed=5).clone()
        out[flags] = (y, loss, eng.grads.clone(), eng.ws_tensor("d1").clone(), eng.ws_tensor("bn1s1").clone())
        del eng
    (y0, l0, g0, d0, s0), (y1, l1, g1, d1, s1) = out[0], out[native.FLAG_BLOCK1_KERNELS]
    assert torch.equal(d0, d1)                                            # the depthwise outputs: the same chain
    assert float((s0 - s1).abs().max()) <= 1e-5 * float(s1.abs().max())  # BatchNorm-1 state: sums in another order
    tol = 1e-5 if precision == "fp32" else 2e-2
    assert torch.isfinite(g0).all() and float((y0 - y1).abs().max()) <= tol and float(((l0 - l1).abs() / l1.abs().clamp_min(1.0)).max()) <= tol
    rel = float((g0.double() - g1.double()).norm() / g1.double().norm())
    print("block 1 folded vs stand-alone (%s): max |dy| %.3g, gradient rel L2 %.3g" % (precision, float((y0 - y1).abs().max()), rel))
    assert rel < (1e-3 if precision == "fp32" else 0.3), rel


@pytest.mark.parametrize("precision", ["fp32", "bf16s"])
def test_localisation_net_per_sample_kernels_equal_the_standalone_kernels(precision):
    """The spatial transformer's localisation net as one workgroup per sample (default, round 4) against its stand-alone kernels
    (CRNN_FLAG_LOC_NET_KERNELS): the same forward bit for bit -- hence the same posteriors, loss and every gradient outside the localisation net --
    and the localisation net's eight parameter gradients to summation order."""
    from crnn_mi355x import native
    B, imgh, imgw, ncls, max_len, tds, u = 6, 100, 32, 38, 23, 128, 256
    cfg = M.Config(imgh=imgh, imgw=imgw, max_len=max_len, time_dense_size=tds, n_units=u, num_classes=ncls)
    p, bn = M.init_params(cfg, seed=6, dtype=np.float64)
    p = M.randomize_params(cfg, p)
    x, lab, il, ll = M.synthetic_batch(cfg, B, seed=4, dtype=np.float64)
    out = {}
    for flags in (0, native.FLAG_LOC_NET_KERNELS):
        eng = Engine(B, imgh, imgw, ncls, max_len, tds, u, stn=True, dropout=True, precision=precision, flags=flags)
        eng.set_params(p, bn)
        eng.ws.fill_(float("nan")); eng.grads.zero_()
        y = eng.forward(x.astype(np.float32), train=True, seed=5).clone()
        loss = eng.backward(lab, il, ll, seed=5).clone()
        out[flags] = (y, loss, eng.grads.clone(), eng.ws_tensor("theta").clone())
        lay = eng.layout
        del eng
    (y0, l0, g0, t0), (y1, l1, g1, t1) = out[0], out[native.FLAG_LOC_NET_KERNELS]
    assert torch.equal(t0, t1) and torch.equal(y0, y1) and torch.equal(l0, l1) and torch.isfinite(g0).all()
    stn = torch.zeros_like(g0, dtype=torch.bool)
    for name, (off, size, _) in lay.items():
        if name.startswith("stn_"):
            stn[off:off + size] = True
            a, b = g0[off:off + size], g1[off:off + size]
            assert float(b.abs().max()) > 0, name
            assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max()) + 1e-7, (name, float((a - b).abs().max()), float(b.abs().max()))
    assert torch.equal(g0[~stn], g1[~stn])


@pytest.mark.parametrize("dropout", [True, False])
def test_fp32_row_stream_schedules_equal_the_tile_schedule(dropout):
    """Parity mode (fp32 tensors), round 4: the depthwise stage runs on the fp32 forms of the row-stream kernels -- forward with the BatchNorm-1
    statistics per workgroup band, backward as one kernel (BatchNorm-1 backward pass 2 + both depthwise gradients) -- and the block
    outputs (round 6: of the pooled blocks too, from q at each window's arg-max) are formed inside the next block's depthwise kernels, which also take BatchNorm-2's backward statistics (the default schedule).
    Against the schedule switches: CRNN_FLAG_NO_BN2_DW_FUSION (block outputs materialised, statistics pass of its own) gives the same forward and
    data gradients, the BatchNorm-2 backward statistics being the same sums in another order; on top of it CRNN_FLAG_NO_DW_BWD_FUSION (the
    three-kernel backward) gives the same bits everywhere but the depthwise weight gradients (partial sums grouped differently);
    CRNN_FLAG_DW_TILE_KERNEL (halo-tile kernels: statistics per tile) agrees to fp32 summation noise."""
    from crnn_mi355x import native
    B, imgh, imgw, ncls, max_len, tds, u = 4, 100, 32, 38, 23, 128, 256
    cfg = M.Config(imgh=imgh, imgw=imgw, max_len=max_len, time_dense_size=tds, n_units=u, num_classes=ncls)
    p, bn = M.init_params(cfg, seed=6, dtype=np.float64)
    p = M.randomize_params(cfg, p)
    x, lab, il, ll = M.synthetic_batch(cfg, B, seed=4, dtype=np.float64)
    out = {}
    N = native.FLAG_NO_BN2_DW_FUSION
    for flags in (0, N, N | native.FLAG_NO_DW_BWD_FUSION, native.FLAG_DW_TILE_KERNEL):
        eng = Engine(B, imgh, imgw, ncls, max_len, tds, u, stn=True, dropout=dropout, precision="fp32", flags=flags)
        assert [eng.lib.crnn_block_output_fused(eng._c, i) for i in range(1, 8)] == ([1, 1, 1, 1, 1, 1, 0] if flags == 0 else [0] * 7)   # (round 6: the pooled blocks 3 and 5 too, from q at the windows' arg-max)
        eng.set_params(p, bn)
        eng.ws.fill_(float("nan")); eng.grads.zero_()
        y = eng.forward(x.astype(np.float32), train=True, seed=5).clone()
        loss = eng.backward(lab, il, ll, seed=5).clone()
        out[flags] = (y, loss, eng.grads.clone())
        lay = eng.layout
        del eng
    y0, l0, g0 = out[N]
    assert torch.isfinite(g0).all()
    y1, l1, g1 = out[N | native.FLAG_NO_DW_BWD_FUSION]
    assert torch.equal(y0, y1) and torch.equal(l0, l1)
    dw = torch.zeros_like(g0, dtype=torch.bool)
    for name, (off, size, _) in lay.items():
        if name.endswith("_dw") and name != "b1_dw":
            dw[off:off + size] = True
            a, b = g0[off:off + size], g1[off:off + size]
            assert float((a - b).abs().max()) <= 2e-5 * float(a.abs().max()) + 1e-7, name
    assert torch.equal(g0[~dw], g1[~dw]), "three-kernel depthwise-stage backward: a data gradient changed"
    y3, l3, g3 = out[0]
    assert torch.equal(y0, y3) and torch.equal(l0, l3) and torch.isfinite(g3).all(), "BatchNorm-2 prologue fusion changed the forward"
    rel = float((g3.double() - g0.double()).norm() / g0.double().norm())
    print("fp32 BatchNorm-2 fusion on/off: gradient rel L2 %.3g" % rel)
    assert rel < 1e-4, rel
    y4, l4, g4 = out[native.FLAG_DW_TILE_KERNEL]
    rel4 = float((g4.double() - g0.double()).norm() / g0.double().norm())
    print("fp32 row-stream vs tile schedule: max |dy| %.3g, gradient rel L2 %.3g" % (float((y0 - y4).abs().max()), rel4))
    assert float((y0 - y4).abs().max()) < 1e-4 and rel4 < 5e-2      # (gate decisions next to a threshold may differ: the bf16 test's bound)


@pytest.mark.parametrize("flags", [0, 65536])    # default (two-plane backward) | CRNN_FLAG_THREE_PLANE_BACKWARD
@pytest.mark.parametrize("shape", [(5, 60, 48, 20, 10, 64, 128), (4, 100, 32, 38, 23, 128, 256)])
def test_parity_mode_resident_weight_kernels_equal_the_tile_schedule_up_to_summation_order(shape, flags):
    """Parity mode, round 6: the pointwise convolutions with a reduction of at most 256 channels run their forward product and data gradient on the
    weights-resident plane kernels (gemm_wres3.hip); CRNN_FLAG_GEMM_TILE_KERNELS keeps gemm_x3p_kernel.  Same planes, same products, another order of the
    fp32 accumulation (four interleaved chains per output) and of the statistics' partial sums: posteriors within 2e-6, loss within 1e-5 relative, the
    gradient within 5e-2 in the norm (a ReLU6 / pooling decision next to its threshold may flip between the schedules: the bound of the other schedule
    tests; the per-kernel tests in test_gpu_ops.py bound the kernels themselves at 2e-6)."""
    from crnn_mi355x import native
    B, imgh, imgw, ncls, max_len, tds, u = shape
    cfg = M.Config(imgh=imgh, imgw=imgw, max_len=max_len, time_dense_size=tds, n_units=u, num_classes=ncls)
    p, bn = M.init_params(cfg, seed=8, dtype=np.float64)
    p = M.randomize_params(cfg, p)
    x, lab, il, ll = M.synthetic_batch(cfg, B, seed=2, dtype=np.float64)
    out = {}
    for fl in (flags, flags | native.FLAG_GEMM_TILE_KERNELS):
        eng = Engine(B, imgh, imgw, ncls, max_len, tds, u, stn=True, dropout=True, precision="fp32", flags=fl)
        eng.set_params(p, bn)
        eng.ws.fill_(float("nan")); eng.grads.zero_()
        y = eng.forward(x.astype(np.float32), train=True, seed=9).clone()
        loss = eng.backward(lab, il, ll, seed=9).clone()
        out[fl] = (y, loss, eng.get_grads())
        del eng
    (y0, l0, g0), (y1, l1, g1) = out[flags], out[flags | native.FLAG_GEMM_TILE_KERNELS]
    assert float((y0 - y1).abs().max()) < 2e-6, float((y0 - y1).abs().max())
    assert float(((l0 - l1).abs() / l1.abs().clamp(min=1.0)).max()) < 1e-5
    worst, num, den = 0.0, 0.0, 0.0
    for k in g0:
        a, b = np.asarray(g0[k], dtype=np.float64), np.asarray(g1[k], dtype=np.float64)
        assert np.isfinite(a).all()
        worst = max(worst, np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))
        num += ((a - b) ** 2).sum(); den += (b ** 2).sum()
    rel = float(np.sqrt(num / den))
    print("resident vs tile schedule: max |dy| %.3g, gradient rel L2 %.3g, worst tensor %.3g of its maximum" % (float((y0 - y1).abs().max()), rel, worst))
    assert rel < 5e-2 and worst < 0.2, (rel, worst)      # (a 1e-7 difference in q flips a few gate / arg-max decisions of this 4-5 sample net: the other schedule tests' bound)


@pytest.mark.parametrize("shape", [(5, 60, 48, 20, 10, 64, 128), (4, 100, 32, 38, 23, 128, 256)])
def test_parity_mode_two_plane_backward_gemms_stay_within_1e_4_of_three_planes(shape):
    """Parity mode: the backward GEMMs (weight and data gradients of the six pointwise convolutions, the dense layers and the RNN projections) carry
    two bf16 planes per operand by default (16 significant bits per factor, half the MFMA work), the forward three.  Against
    CRNN_FLAG_THREE_PLANE_BACKWARD: the same forward bit for bit -- posteriors, loss, hence every gate decision -- and gradients within 1e-4 of
    the norm (measured 1e-5; tensor by tensor within 1e-3 of the tensor's largest element, measured 1e-4 on the tensor with the most cancellation).  CRNN_FLAG_TWO_PLANE_FORWARD (opt-in) moves the posteriors by < 1e-4 and the CTC costs by < 1e-4
    relative, with identical greedy decodes."""
    from crnn_mi355x import native
    B, imgh, imgw, ncls, max_len, tds, u = shape
    cfg = M.Config(imgh=imgh, imgw=imgw, max_len=max_len, time_dense_size=tds, n_units=u, num_classes=ncls)
    p, bn = M.init_params(cfg, seed=12, dtype=np.float64)
    p = M.randomize_params(cfg, p)
    x, lab, il, ll = M.synthetic_batch(cfg, B, seed=6, dtype=np.float64)
    out = {}
    for flags in (0, native.FLAG_THREE_PLANE_BACKWARD, native.FLAG_TWO_PLANE_FORWARD | native.FLAG_THREE_PLANE_BACKWARD):
        eng = Engine(B, imgh, imgw, ncls, max_len, tds, u, stn=True, dropout=True, precision="fp32", flags=flags)
        eng.set_params(p, bn)
        eng.ws.fill_(float("nan")); eng.grads.zero_()
        y = eng.forward(x.astype(np.float32), train=True, seed=3).clone()
        loss = eng.backward(lab, il, ll, seed=3).clone()
        dec = eng.greedy_decode()[0].clone()
        out[flags] = (y, loss, eng.grads.clone(), dec)
        lay = eng.layout
        del eng
    (y2, l2, g2, d2), (y3, l3, g3, d3) = out[0], out[native.FLAG_THREE_PLANE_BACKWARD]
    assert torch.isfinite(g2).all() and torch.equal(y2, y3) and torch.equal(l2, l3) and torch.equal(d2, d3), "the forward must not depend on the backward's planes"
    rel = float((g2.double() - g3.double()).norm() / g3.double().norm())
    assert 0 < rel < 1e-4, rel
    worst = 0.0
    for name, (off, size, _) in lay.items():
        a, b = g2[off:off + size].double(), g3[off:off + size].double()
        if float(b.abs().max()) > 0:
            worst = max(worst, float((a - b).abs().max() / b.abs().max()))
    print("two-plane backward: gradient rel L2 %.3g, worst tensor max-rel %.3g" % (rel, worst))
    assert worst < 1e-3, worst
    yf, lf, gf, df = out[native.FLAG_TWO_PLANE_FORWARD | native.FLAG_THREE_PLANE_BACKWARD]
    dy = float((yf - y3).abs().max()); dl = float(((lf - l3).abs() / l3.abs().clamp_min(1.0)).max())
    print("two-plane forward: max |dy| %.3g, max rel dloss %.3g" % (dy, dl))
    assert 0 < dy < 1e-4 and dl < 1e-4 and torch.equal(df, d3), (dy, dl)


@pytest.mark.parametrize("shape", [(4, 100, 32, 38, 23, 128, 256), (8, 100, 32, 38, 23, 128, 256), (3, 200, 32, 62, 21, 128, 256)])
def test_parity_mode_gradient_planes_schedule_equals_the_fp32_gradient_schedule(shape):
    """Parity mode, round 6: BatchNorm-2's input gradient of blocks 3-7 is written as two bf16 planes by the BatchNorm backward and read as such by the block's
    data-gradient GEMM (crnn_gemm_pres_bnstats: LDS-DMA, weight planes resident) and weight-gradient GEMM (crnn_pwconv_bnrelu6_wgrad_planes_stream_gp).
    CRNN_FLAG_NO_GRADIENT_PLANES keeps the fp32 tensor that both GEMMs split while staging (rounds 4-5).  Same planes, same products: the forward is untouched
    (bit-identical posteriors / loss) and every gradient tensor agrees to the order of fp32 sums (the data gradients are the tile kernel's bit for bit, the
    statistics and the weight gradients the same sums grouped differently) -- within 1e-4 of each tensor's maximum (measured 2e-6 .. 3e-5, on BatchNorm
    shift gradients, the sums with the most cancellation): the level of the two-plane products themselves."""
    from crnn_mi355x import native
    B, imgh, imgw, ncls, max_len, tds, u = shape
    cfg = M.Config(imgh=imgh, imgw=imgw, max_len=max_len, time_dense_size=tds, n_units=u, num_classes=ncls)
    p, bn = M.init_params(cfg, seed=12, dtype=np.float64)
    p = M.randomize_params(cfg, p)
    x, lab, il, ll = M.synthetic_batch(cfg, B, seed=6, dtype=np.float64)
    out = {}
    for flags in (0, native.FLAG_NO_GRADIENT_PLANES):
        eng = Engine(B, imgh, imgw, ncls, max_len, tds, u, stn=True, dropout=True, precision="fp32", flags=flags)
        eng.set_params(p, bn)
        eng.ws.fill_(float("nan")); eng.grads.zero_()
        y = eng.forward(x.astype(np.float32), train=True, seed=3).clone()
        loss = eng.backward(lab, il, ll, seed=3).clone()
        out[flags] = (y, loss, eng.grads.clone())
        lay = eng.layout
        del eng
    (y0, l0, g0), (y1, l1, g1) = out[0], out[native.FLAG_NO_GRADIENT_PLANES]
    assert torch.isfinite(g0).all() and torch.equal(y0, y1) and torch.equal(l0, l1)
    worst, wname = 0.0, ""
    for name, (off, size, _) in lay.items():
        a, b = g0[off:off + size].double(), g1[off:off + size].double()
        if float(b.abs().max()) > 0:
            r = float((a - b).abs().max() / b.abs().max())
            if r > worst: worst, wname = r, name
    print("gradient planes vs fp32 gradient tensors: worst tensor %s max-rel %.3g" % (wname, worst))
    assert worst < 1e-4, (wname, worst)


@pytest.mark.parametrize("precision", ["fp32", "bf16s"])
@pytest.mark.parametrize("shape", [(4, 100, 32, 38, 23, 128, 256), (3, 200, 32, 62, 21, 128, 256)])
def test_pooled_blocks_statistics_from_saved_window_maxima_are_bit_identical(shape, precision):
    """Round 6: the training forward keeps q at each pool window's arg-max for blocks 3 and 5 and BatchNorm-2's backward takes its statistics from those values
    (one read per window instead of the window).  CRNN_FLAG_NO_POOL_ARGMAX_Q scans the windows again (rounds 1-5).  bf16 tensors: same sums in the same order --
    posteriors, losses and every gradient are bit-identical.  fp32 tensors (where the BatchNorm-2 prologue fusion is the default): the saved maxima also replace
    the pooled block's OUTPUT -- block i + 1's depthwise kernels form it from them in LDS, forward and backward, and the backward one takes the statistics: the
    forward is bit-identical, the gradients agree to the order of fp32 sums."""
    from crnn_mi355x import native
    B, imgh, imgw, ncls, max_len, tds, u = shape
    cfg = M.Config(imgh=imgh, imgw=imgw, max_len=max_len, time_dense_size=tds, n_units=u, num_classes=ncls)
    p, bn = M.init_params(cfg, seed=12, dtype=np.float64)
    p = M.randomize_params(cfg, p)
    x, lab, il, ll = M.synthetic_batch(cfg, B, seed=6, dtype=np.float64)
    out = {}
    for flags in (0, native.FLAG_NO_POOL_ARGMAX_Q):
        eng = Engine(B, imgh, imgw, ncls, max_len, tds, u, stn=True, dropout=True, precision=precision, flags=flags)
        eng.set_params(p, bn)
        eng.ws.fill_(float("nan")); eng.grads.zero_()
        y = eng.forward(x.astype(np.float32), train=True, seed=3).clone()
        loss = eng.backward(lab, il, ll, seed=3).clone()
        out[flags] = (y, loss, eng.grads.clone())
        del eng
    (y0, l0, g0), (y1, l1, g1) = out[0], out[native.FLAG_NO_POOL_ARGMAX_Q]
    assert torch.isfinite(g0).all() and float(g0.abs().max()) > 0
    assert torch.equal(y0, y1) and torch.equal(l0, l1)
    if precision == "bf16s":
        assert torch.equal(g0, g1)
    else:   # fp32 tensors: the saved maxima also stand in for q in the next block's prologue kernels, whose backward takes the statistics (another order of the sums)
        rel = float((g0.double() - g1.double()).norm() / g1.double().norm())
        print("pooled blocks through the prologue kernels: gradient rel L2 %.3g" % rel)
        assert rel < 1e-5, rel


@pytest.mark.parametrize("shape", [(5, 60, 48, 20, 10, 64, 128), (4, 100, 32, 38, 23, 128, 256)])
def test_bf16s_schedule_switches_match_the_two_pass_path(shape):
    """bf16s training applies the depthwise BatchNorm + ReLU6 inside the pointwise GEMMs (forward and weight gradient);
    crnn_config.flags bit CRNN_FLAG_NO_DW_BN_FUSION materialises the activated tensor instead.  Same operands, same order of
    operations: posteriors, losses and every gradient are bit-identical.  The same holds for the other schedule switches on the
    tile GEMM (CRNN_FLAG_GEMM_TILE_KERNELS): LSTM recurrences as per-step launches (CRNN_FLAG_RNN_STEP_KERNELS), the unfused
    depthwise-stage backward (CRNN_FLAG_NO_DW_BWD_FUSION; its depthwise weight gradients group their partial sums differently).
    The default schedule runs the pointwise convolutions on the weights-resident kernels: products and data gradients are the
    same bits, but the BatchNorm-2 statistics are summed in another order (per IO wave over the launch instead of per 128-row
    tile), and the depthwise forward on the row-stream kernel (CRNN_FLAG_DW_TILE_KERNEL switches it off: same outputs, BatchNorm-1
    statistics per workgroup band instead of per halo tile), so against the tile schedules everything agrees to the bf16 storage's
    rounding noise, not bit for bit -- bounds below."""
    from crnn_mi355x import native
    B, imgh, imgw, ncls, max_len, tds, u = shape
    cfg = M.Config(imgh=imgh, imgw=imgw, max_len=max_len, time_dense_size=tds, n_units=u, num_classes=ncls)
    p, bn = M.init_params(cfg, seed=6, dtype=np.float64)
    p = M.randomize_params(cfg, p)
    x, lab, il, ll = M.synthetic_batch(cfg, B, seed=4, dtype=np.float64)
    out = {}
    T = native.FLAG_GEMM_TILE_KERNELS | native.FLAG_DW_TILE_KERNEL
    for flags in (T, T | native.FLAG_NO_DW_BN_FUSION, T | native.FLAG_RNN_STEP_KERNELS, T | native.FLAG_NO_DW_BWD_FUSION, native.FLAG_BN2_DW_FUSION,
                  native.FLAG_BN2_DW_FUSION | native.FLAG_BN2_STATS_FUSION, native.FLAG_NO_BN_STATS_FUSION, 0):
        eng = Engine(B, imgh, imgw, ncls, max_len, tds, u, stn=True, dropout=True, precision="bf16s", flags=flags)
        eng.set_params(p, bn)
        eng.ws.fill_(float("nan")); eng.grads.zero_()
        y = eng.forward(x.astype(np.float32), train=True, seed=5).clone()
        loss = eng.backward(lab, il, ll, seed=5).clone()
        out[flags] = (y, loss, eng.grads.clone())
        del eng
    lay = Engine(B, imgh, imgw, ncls, max_len, tds, u, precision="bf16s").layout
    y0, l0, g0 = out[T]
    # default schedule with / without the BatchNorm-backward statistics inside the data-gradient GEMM: same forward, same data gradients;
    # the statistics are the same sums in another order, so the gradients agree to fp32 summation noise re-rounded through bf16 tensors
    ya, la, ga = out[native.FLAG_NO_BN_STATS_FUSION]; yb, lb, gb = out[0]
    assert torch.equal(ya, yb) and torch.equal(la, lb)
    rel = float((ga.double() - gb.double()).norm() / ga.double().norm())
    print("BatchNorm-statistics fusion on/off: gradient rel L2 %.3g" % rel)
    assert torch.isfinite(ga).all() and rel < 5e-2, rel
    # block outputs formed inside the next block's depthwise row-stream kernels (opt-in CRNN_FLAG_BN2_DW_FUSION, where the shape rules hold: image
    # width 32) or materialised by crnn_bn_act_pool_drop_ex (default): same arithmetic, same summation orders -- everything bit-identical
    yd, ld, gd_ = out[native.FLAG_BN2_DW_FUSION]; ye, le, ge = out[native.FLAG_BN2_DW_FUSION | native.FLAG_BN2_STATS_FUSION]
    assert torch.equal(yd, yb) and torch.equal(ld, lb) and torch.equal(gd_, gb), "BatchNorm-2 prologue fusion changed the results"
    # ... and the statistics pass of those BatchNorms' backward inside the next block's depthwise-stage backward (opt-in: CRNN_FLAG_BN2_STATS_FUSION)
    # or as a kernel of its own (default): same forward, the statistics are the same sums in another order
    assert torch.equal(ye, yb) and torch.equal(le, lb)
    rel2 = float((ge.double() - gb.double()).norm() / ge.double().norm())
    print("BatchNorm-2 statistics fusion on/off: gradient rel L2 %.3g" % rel2)
    assert torch.isfinite(ge).all() and rel2 < 5e-2, rel2
    for flags in (T | native.FLAG_NO_DW_BN_FUSION, T | native.FLAG_RNN_STEP_KERNELS, T | native.FLAG_NO_DW_BWD_FUSION):
        y1, l1, g1 = out[flags]
        assert torch.isfinite(g1).all() and torch.equal(y0, y1) and torch.equal(l0, l1), flags
        if flags == T | native.FLAG_RNN_STEP_KERNELS:
            # the persistent LSTM backward also sums its dz over time per 16-row batch tile for the recurrent biases (round 4); the step kernels' path
            # sums the stored dz in column-reduction chunks: the four bias gradients to summation round-off, everything else exactly
            rb = torch.zeros_like(g0, dtype=torch.bool)
            for name, (off, size, _) in lay.items():
                if name.startswith("rnn") and name.endswith("_b"):
                    rb[off:off + size] = True
                    a, b = g0[off:off + size], g1[off:off + size]
                    assert float((a - b).abs().max()) <= 2e-5 * float(a.abs().max()) + 1e-7, name
            assert torch.equal(g0[~rb], g1[~rb]), flags
        elif flags != T | native.FLAG_NO_DW_BWD_FUSION:
            assert torch.equal(g0, g1), flags
        else:
            # the fused depthwise-stage backward groups the partial sums of the depthwise weight gradients differently: those six
            # tensors agree to summation round-off, every other gradient (all data gradients are bit-identical) exactly
            dw = torch.zeros_like(g0, dtype=torch.bool)
            for name, (off, size, _) in lay.items():
                if name.endswith("_dw") and name != "b1_dw":
                    dw[off:off + size] = True
                    a, b = g0[off:off + size], g1[off:off + size]
                    assert float((a - b).abs().max()) <= 2e-4 * float(a.abs().max()) + 1e-6, name
            assert torch.equal(g0[~dw], g1[~dw])
    # default schedule (weights-resident pointwise kernels) against the tile schedule
    y1, l1, g1 = out[0]
    assert torch.isfinite(g1).all()
    dy = float((y0 - y1).abs().max()); dl = float(((l0 - l1).abs() / l0.abs().clamp_min(1.0)).max())
    worst = ("", 0.0)
    for name, (off, size, _) in lay.items():
        a, b = g0[off:off + size].double(), g1[off:off + size].double()
        scale = float(a.norm())
        if "_bn" in name:
            # d(gamma) and d(beta) of one BatchNorm layer are sums over the same B*H*W terms: a sum that cancels to a small value (block 1 has ONE channel: its
            # d(beta) is a single cancelling number) is judged against the larger of the pair, as check_case does, not against itself
            o2, s2, _ = lay[name[:-1] + ("b" if name.endswith("g") else "g")]
            scale = max(scale, float(g0[o2:o2 + s2].double().norm()))
        e = float((a - b).norm() / (scale + 1e-30))
        if size < 4:
            continue   # block 1's one-channel BatchNorm: d(gamma) and d(beta) are single sums of B*H*W terms that BOTH cancel (measured 1.57 relative: a
            #            scalar judged against itself); they count in the whole-gradient figure below
        if e > worst[1]: worst = (name, e)
    glob = float((g0.double() - g1.double()).norm() / g0.double().norm())
    print("default vs tile schedule: max |dy| %.3g, max rel dloss %.3g, gradient rel L2 %.3g, worst tensor %s %.3g" % (dy, dl, glob, worst[0], worst[1]))
    # measured (round 5, both shapes): |dy| 6.5e-4 .. 7.3e-4, dloss 3.3e-4 .. 4.5e-4, whole gradient 0.18 .. 0.22, worst single tensor 0.20 (stn_d2_w) / 0.67 (b1_pw), at the far
    # end of the backward chain, once a BatchNorm layer's cancelling d(beta) is judged against its d(gamma) and block 1's one-channel BatchNorm
    # (two cancelling scalars, 1.57 relative) is left to the whole-gradient figure: statistics that differ in the last fp32 bits re-round a few bf16 activations, and this random-weight 4..5-sample net amplifies that like it
    # amplifies the bf16 storage itself (bf16s against the fp64 oracle: ~5e-2, test above).  An uncorrelated or sign-flipped tensor would read >= 1.
    # (the 100x32 shape: worst tensor b1_pw 0.67 -- 64 cancelling sums at the very end of the chain, cosine 0.75; an uncorrelated tensor reads 1.41, a
    # sign-flipped one 2.0: the bound sits between)
    # (round 6: what bounds the GRADIENTS of either schedule is test_bf16s_training_step_gradients_under_the_device_decisions -- the fp64 oracle's backward under
    # each schedule's own decisions, per tensor; this comparison of two chaotic forwards only guards against a schedule going wild)
    assert dy < 5e-3 and dl < 2e-3 and glob < 0.3 and worst[1] < 1.0, (dy, dl, glob, worst)


@pytest.mark.parametrize("precision", ["fp32", "bf16s"])
def test_gru_model_persistent_recurrences_equal_the_step_kernels(precision):
    """GRU variant (what the reference's train.py builds): the whole train step with the persistent recurrences (default) must equal
    the per-step-launch schedule (CRNN_FLAG_RNN_STEP_KERNELS) bit for bit -- posteriors, losses, every gradient but the recurrent biases' -- and so must the
    BPTT launches on the linear workgroup -> cluster map (CRNN_FLAG_RNN_LINEAR_CLUSTERS)."""
    from crnn_mi355x import native
    B, imgh, imgw, ncls, max_len, tds, u = 20, 60, 32, 38, 10, 64, 256
    cfg = M.Config(imgh=imgh, imgw=imgw, max_len=max_len, time_dense_size=tds, n_units=u, num_classes=ncls, gru=True)
    p, bn = M.init_params(cfg, seed=8, dtype=np.float64)
    p = M.randomize_params(cfg, p)
    x, lab, il, ll = M.synthetic_batch(cfg, B, seed=2, dtype=np.float64)
    out = {}
    for flags in (0, native.FLAG_RNN_STEP_KERNELS, native.FLAG_RNN_LINEAR_CLUSTERS):
        eng = Engine(B, imgh, imgw, ncls, max_len, tds, u, gru=True, stn=True, dropout=True, precision=precision, flags=flags)
        eng.set_params(p, bn)
        eng.grads.zero_()
        y = eng.forward(x.astype(np.float32), train=True, seed=5).clone()
        loss = eng.backward(lab, il, ll, seed=5).clone()
        eng.check_rnn_status()
        assert (eng._rnn_giveups is not None) == (flags != native.FLAG_RNN_STEP_KERNELS)
        out[flags] = (y, loss, eng.grads.clone())
        del eng
    y0, l0, g0 = out[0]
    assert torch.isfinite(g0).all() and float(g0.abs().max()) > 0
    lay = Engine(B, imgh, imgw, ncls, max_len, tds, u, gru=True, precision=precision).layout
    for flags in list(out)[1:]:
        y1, l1, g1 = out[flags]
        assert torch.equal(y0, y1) and torch.equal(l0, l1), flags
        if flags == native.FLAG_RNN_STEP_KERNELS:
            # (round 4) the persistent backward sums its dz per 16-row batch tile for the recurrent biases, the step kernels' path reduces the stored dz
            # in column chunks: those four gradients to summation round-off, everything else bit for bit
            rb = torch.zeros_like(g0, dtype=torch.bool)
            for name, (off, size, _) in lay.items():
                if name.startswith("rnn") and name.endswith("_b"):
                    rb[off:off + size] = True
                    a, b = g0[off:off + size], g1[off:off + size]
                    assert float((a - b).abs().max()) <= 2e-5 * float(a.abs().max()) + 1e-7, name
            assert torch.equal(g0[~rb], g1[~rb]), flags
        else:
            assert torch.equal(g0, g1), flags


def test_parity_mode_three_plane_gemms_track_the_fp32_mfma_path():
    """The parity mode's GEMMs are three-plane bf16 products (crnn_gemm_f32x3); CRNN_FLAG_F32_MFMA_GEMMS puts them on the fp32 MFMA (an fmaf chain
    bit for bit, the path the oracle comparisons of round 1-2 ran on).  The two must agree to fp32 round-off: posteriors within 1e-5, CTC costs within 1e-5 relative, identical greedy decode.  The gradient
    is bounded like every gradient comparison between two forwards that differ in the last bits: a handful of ReLU6 /
    max-pool decisions within round-off of their threshold flip and move per-channel sums by percents -- measured 4.6e-3 of the norm."""
    from crnn_mi355x import native
    B, imgh, imgw, ncls, max_len, tds, u = 8, 100, 32, 38, 23, 128, 256
    cfg = M.Config(imgh=imgh, imgw=imgw, max_len=max_len, time_dense_size=tds, n_units=u, num_classes=ncls)
    p, bn = M.init_params(cfg, seed=9, dtype=np.float64)
    p = M.randomize_params(cfg, p)
    x, lab, il, ll = M.synthetic_batch(cfg, B, seed=3, dtype=np.float64)
    out = {}
    for flags in (native.FLAG_F32_MFMA_GEMMS, 0):
        eng = Engine(B, imgh, imgw, ncls, max_len, tds, u, stn=True, dropout=False, precision="fp32", flags=flags)
        eng.set_params(p, bn)
        eng.grads.zero_()
        y = eng.forward(x.astype(np.float32), train=True, seed=1).clone()
        loss = eng.backward(lab, il, ll, seed=1).clone()
        dec = eng.greedy_decode()[0].clone()
        out[flags] = (y, loss, eng.grads.clone(), dec)
        del eng
    (y0, l0, g0, d0), (y1, l1, g1, d1) = out[native.FLAG_F32_MFMA_GEMMS], out[0]
    dy = float((y0 - y1).abs().max()); dl = float(((l0 - l1).abs() / l0.abs().clamp_min(1.0)).max())
    dg = float((g0.double() - g1.double()).norm() / g0.double().norm())
    print("three-plane vs fp32 MFMA: max |dy| %.3g, max rel dloss %.3g, gradient rel L2 %.3g" % (dy, dl, dg))
    assert torch.isfinite(g1).all() and dy < 1e-5 and dl < 1e-5 and dg < 3e-2 and torch.equal(d0, d1), (dy, dl, dg)


def test_small_model_stn_disabled():
    check_case(run_case(B=3, imgh=40, imgw=32, u=64, tds=32, max_len=6, stn=False, dropout=False), "nostn")


def test_config1_shape_full_model_step_and_decode():
    """BASELINE config 1 shape (100x32, max_len 23, tds 128, n_units 256) at a small batch: forward, loss, grads,
    one Adam(1e-4, beta1 .5, clipnorm 5) step, BN moving statistics, inference forward and decoders."""
    res = run_case(B=6, imgh=100, imgw=32, u=256, tds=128, max_len=23, stn=True, dropout=False)
    check_case(res, "config1")
    cfg, eng, p, bn, (x, lab, il, ll), yd, loss_d, gd, c, loss_b, g, rep, gdev = res
    # optimizer + BN update
    eng.adam_step(1e-4, 0.5, 0.999, 1e-7, 5.0, iteration=0)
    eng.bn_update()
    opt = M.Adam(lr=1e-4, beta_1=0.5, beta_2=0.999, epsilon=1e-7, clipnorm=5.0)
    # the optimizer arithmetic is checked on the DEVICE's own gradient (gd; its parity with the oracle's is asserted by
    # check_case above): the first Adam step moves a weight by ~lr*g/(|g|+eps'), so feeding the oracle's gradient instead
    # would turn fp32 summation-order noise on near-zero gradient elements into differences of several % of lr
    p_ref = opt.step({k: v.copy() for k, v in p.items()}, {k: gd[k].astype(np.float64) for k in gd})
    pd = eng.get_params()
    for k in p:
        assert np.abs(pd[k] - p_ref[k]).max() < 2e-7 + 2e-6 * np.abs(p_ref[k]).max(), k
    bn_ref = M.bn_update(cfg, {k: v.copy() for k, v in bn.items()}, c)
    bnd = eng.get_bn()
    for k in bn_ref:
        assert np.abs(bnd[k] - bn_ref[k]).max() < 1e-4 * max(1.0, np.abs(bn_ref[k]).max()), k
    # inference-mode forward with the updated weights/statistics; greedy indices bit-exact; beam vs oracle
    y_inf = eng.forward(x.astype(np.float32), train=False).cpu().numpy()
    y_ref, _ = M.forward(cfg, p_ref, bn_ref, x, train=False)
    assert np.abs(y_inf - y_ref).max() < 1e-4
    out, ln = eng.greedy_decode()
    ref, rl = ctc.ctc_greedy_decode(y_ref)
    assert np.array_equal(out.cpu().numpy(), ref) and np.array_equal(ln.cpu().numpy(), rl)
    assert np.array_equal(np.argmax(y_inf, -1), np.argmax(y_ref, -1))
    bo, bl, bs = eng.beam_decode(beam_width=10)
    ro, rl2, rs_ = ctc.ctc_beam_decode(y_inf, beam_width=10)
    assert np.array_equal(bo.cpu().numpy(), ro) and np.array_equal(bl.cpu().numpy(), rl2)


def test_iam_shape_forward_loss():
    """BASELINE config 3 shape: height 32, width 200 (T=102, CTC 100 steps), max_len 21, STN on."""
    res = run_case(B=3, imgh=200, imgw=32, u=128, tds=64, max_len=21, stn=True, dropout=False)
    check_case(res, "iam")


def test_iam_shape_full_width_model_variable_width_text():
    """BASELINE configs[2] at the real model width (n_units 256, time_dense_size 128) on variable-width text lines (random prefix of
    40..200 rows of noise, the rest the modal grey value: SURVEY 8d C3, utils.py:372-400): fp32 parity of every intermediate, logits,
    CTC loss (T = 100 steps) and gradients."""
    res = run_case(B=2, imgh=200, imgw=32, u=256, tds=128, max_len=21, stn=True, dropout=False, variable_width=True)
    check_case(res, "iam-full")


def test_bf16s_inference_at_batch256_against_the_oracle_on_a_slice():
    """The benchmarked storage mode (bf16 conv-stack tensors) at the benchmarked batch (256): inference BatchNorm makes every image
    independent, so the first 16 posteriors can be checked against the fp64 oracle run on those 16 images alone.  Bounds are what
    the mode honestly delivers (measured: max |dy| ~2e-2 on single time steps whose top two classes are close, mean |dy| ~3e-4,
    per-sample CTC cost within ~3e-3 relative, >= 98 % of arg-max indices equal) -- not the 1e-3 parity tolerance, which only
    the fp32 mode meets (test_config1_shape...)."""
    cfg = M.Config()
    B, n = 256, 16
    p, bn = M.init_params(cfg, seed=2, dtype=np.float64)
    p = M.randomize_params(cfg, p)
    rs = np.random.RandomState(4)
    for k in bn:     # non-trivial moving statistics
        bn[k] = (np.abs(rs.normal(size=bn[k].shape)) * 0.5 + 0.5) if k.endswith("_var") else rs.normal(size=bn[k].shape) * 0.1
    x, lab, il, ll = M.synthetic_batch(cfg, B, seed=9, dtype=np.float64)
    y_ref, _ = M.forward(cfg, p, bn, x[:n], train=False)
    loss_ref, _ = ctc.ctc_loss_and_grad(y_ref, lab[:n], il[:n], ll[:n])
    out = {}
    for precision in ("fp32", "bf16s"):
        eng = Engine(B, dropout=False, precision=precision)
        eng.set_params(p, bn)
        y = eng.forward(x.astype(np.float32), train=False).cpu().numpy()[:n]
        loss_d, _ = ctc.ctc_loss_and_grad(y.astype(np.float64), lab[:n], il[:n], ll[:n])
        out[precision] = (float(np.abs(y - y_ref).max()), float(np.abs(y - y_ref).mean()), float((np.argmax(y, -1) == np.argmax(y_ref, -1)).mean()),
                          float(np.abs(loss_d - loss_ref).max() / np.abs(loss_ref).max()))
        print("[batch256 %s] max|dy| %.3e mean|dy| %.3e argmax agreement %.4f rel CTC-cost err %.3e" % ((precision,) + out[precision]))
    assert out["fp32"][0] < 1e-4 and out["fp32"][2] == 1.0 and out["fp32"][3] < 1e-4
    assert out["bf16s"][0] < 4e-2 and out["bf16s"][1] < 1e-3 and out["bf16s"][2] >= 0.98 and out["bf16s"][3] < 6e-3


def test_predict_path_batch1024_properties():
    """BASELINE configs[4] size: inference at batch 1024 + beam search (width 10).  Properties that need no oracle at this size:
    per-image independence (rows 0..7 equal the same images run at batch 8, bit for bit in fp32), normalised posteriors, greedy ==
    arg-max/collapse of the device posteriors, beam search == the CPU restatement of TF's beam search on a sample of rows, and the
    top beam never scores below the greedy path."""
    cfg = M.Config()
    B = 1024
    p, bn = M.init_params(cfg, seed=2, dtype=np.float32)
    p = M.randomize_params(cfg, p)
    x = M.synthetic_batch(cfg, B, seed=11)[0]
    big = Engine(B, dropout=False); big.set_params(p, bn)
    yb = big.forward(x, train=False).clone()
    small = Engine(8, dropout=False); small.set_params(p, bn)
    ys = small.forward(x[:8], train=False)
    assert torch.allclose(yb[:8], ys, rtol=0, atol=2e-6), float((yb[:8] - ys).abs().max())
    y = yb.cpu().numpy()
    assert np.isfinite(y).all() and np.abs(y.sum(-1) - 1).max() < 1e-5
    out, ln = big.greedy_decode()
    ref, rl = ctc.ctc_greedy_decode(y)
    assert np.array_equal(out.cpu().numpy(), ref) and np.array_equal(ln.cpu().numpy(), rl)
    bo, bl, bs = big.beam_decode(beam_width=10)
    bo, bl, bs = bo.cpu().numpy(), bl.cpu().numpy(), bs.cpu().numpy()
    rows = np.r_[0:12, 500:506, 1018:1024]
    ro, rl2, rsc = ctc.ctc_beam_decode(y[rows], beam_width=10)
    assert np.array_equal(bo[rows], ro) and np.array_equal(bl[rows], rl2)
    assert np.all(np.isfinite(bs)) and (bl >= 0).all() and (bl <= big.T).all()


def test_train_steps_are_deterministic_and_loss_decreases():
    cfg = M.Config()
    B = 16
    p, bn = M.init_params(cfg, seed=1, dtype=np.float32)
    x, lab, il, ll = M.synthetic_batch(cfg, B, seed=0)
    from crnn_mi355x.optimizers import Adam
    losses = []
    for rep in range(2):
        eng = Engine(B, dropout=True)
        eng.set_params(p, bn)
        opt = Adam(lr=1e-3, beta_1=0.5, beta_2=0.999, clipnorm=5)
        ls = []
        for it in range(12):
            ls.append(float(eng.train_step(x, lab, il, ll, opt, it).mean().item()))
        losses.append(ls)
        final = eng.params.clone()
        if rep == 0:
            first = final
    assert losses[0] == losses[1], "train step is not run-to-run deterministic"
    assert torch.equal(first, final)
    assert np.isfinite(losses[0]).all() and losses[0][-1] < losses[0][0]


@pytest.mark.parametrize("precision", ["bf16", "bf16s"])
def test_bf16_mfma_mode_tracks_the_fp32_oracle(precision):
    """Fast modes: 'bf16' = GEMM products in bf16 (fp32 tensors); 'bf16s' = additionally bf16 conv-stack tensors in HBM.
    Not parity modes: the forward must stay within bf16 round-off of the oracle and the gradients must point the same way."""
    cfg = M.Config()
    B = 8
    p, bn = M.init_params(cfg, seed=7, dtype=np.float64)
    p = M.randomize_params(cfg, p)
    x, lab, il, ll = M.synthetic_batch(cfg, B, seed=1, dtype=np.float64)
    eng = Engine(B, dropout=False, precision=precision)
    eng.set_params(p, bn)
    yd = eng.forward(x.astype(np.float32), train=True, seed=0).cpu().numpy()
    loss_d = eng.backward(lab, il, ll, seed=0).cpu().numpy()
    gd = eng.get_grads()
    loss, loss_b, g, c = M.loss_and_grads(cfg, p, bn, x, lab, il, ll)
    err_y = np.abs(yd - c["y_pred"]).max()
    agree = (np.argmax(yd, -1) == np.argmax(c["y_pred"], -1)).mean()
    rel_loss = np.abs(loss_d - loss_b).max() / np.abs(loss_b).max()
    cos = {k: float((gd[k].ravel() @ g[k].ravel()) / (np.linalg.norm(gd[k]) * np.linalg.norm(g[k]) + 1e-30)) for k in p if g[k].size >= 512}
    print(f"[{precision}] max|dy|={err_y:.3e} argmax agreement={agree:.4f} rel loss err={rel_loss:.3e} grad cosines: "
          + " ".join(f"{k}:{v:.3f}" for k, v in cos.items()))
    assert err_y < 5e-2 and agree > (0.97 if precision == "bf16" else 0.93) and rel_loss < 2e-2
    # bf16 products perturb ~1 % of the ReLU6 / pool decisions (cf. DESIGN.md "threshold flips"), so the gradients
    # of the lower layers are noisy copies of the fp64 ones; the top of the network must still agree closely
    for k in ("dense2_w", "rnn2f_w", "rnn2b_u", "rnn1f_w", "dense1_w"):
        assert cos[k] > (0.97 if precision == "bf16" else 0.95), (k, cos[k])
    # (the STN gradients sit below seven blocks of flip noise: their cosine moves between 0.45 and 0.7 with any change of
    # rounding anywhere above them, in either bf16 mode)
    assert min(cos.values()) > 0.3, cos      # (direction only; the per-tensor BOUND of the bf16s backward: test_bf16s_training_step_gradients_under_the_device_decisions)
    # what matters for the fast mode: optimisation behaves like the fp32 mode
    from crnn_mi355x.optimizers import Adam
    p32, bn32 = M.init_params(cfg, seed=1, dtype=np.float32)
    xb, labb, ilb, llb = M.synthetic_batch(cfg, 32, seed=0)
    curves = {}
    for prec in ("fp32", precision):
        e = Engine(32, dropout=True, precision=prec)
        e.set_params(p32, bn32)
        # lr 2e-4 (the reference default is 1e-4): at 1e-3 the fp32 run itself is spiky and the comparison turns chaotic
        opt = Adam(lr=2e-4, beta_1=0.5, beta_2=0.999, clipnorm=5)
        curves[prec] = [float(e.train_step(xb, labb, ilb, llb, opt, it).mean().item()) for it in range(30)]
    print(f"[{precision}] loss curves fp32 vs {precision}:", [round(v, 2) for v in curves["fp32"][::6]], [round(v, 2) for v in curves[precision][::6]])
    # single steps with dropout are bumpy (both modes): compare the level of the last steps, not one sample
    tail = {k: float(np.mean(v[-6:])) for k, v in curves.items()}
    assert tail[precision] < 0.8 * curves[precision][0]
    assert abs(tail[precision] - tail["fp32"]) < 0.1 * tail["fp32"], (curves["fp32"][-6:], curves[precision][-6:])


def test_two_stage_backward_equals_single_call():
    """crnn_backward_top + crnn_backward_bottom (the form a data-parallel host overlaps with the all-reduce) must give
    the very same gradient buffer and loss as crnn_backward."""
    cfg = M.Config()
    B = 4
    p, bn = M.init_params(cfg, seed=3, dtype=np.float32)
    p = M.randomize_params(cfg, p)
    x, lab, il, ll = M.synthetic_batch(cfg, B, seed=5)
    for precision in ("fp32", "bf16s"):
        eng = Engine(B, dropout=True, precision=precision)
        eng.set_params(p, bn)
        eng.forward(x, train=True, seed=11)
        loss1 = eng.backward(lab, il, ll, seed=11).clone(); g1 = eng.grads.clone()
        eng.grads.fill_(float("nan"))
        eng.forward(x, train=True, seed=11)
        loss2 = eng.backward_top(lab, il, ll, seed=11).clone()
        split = eng.grad_split
        top_done = eng.grads[split:].clone()
        eng.backward_bottom(seed=11)
        assert 0 < split < eng.grads.numel()
        assert torch.equal(loss1, loss2)
        assert torch.equal(eng.grads, g1), precision
        assert torch.equal(top_done, g1[split:]), "upper-layer gradients must be final after the first stage"


@pytest.mark.parametrize("precision", ["fp32", "bf16s"])
def test_full_size_batch256_properties(precision):
    """BASELINE configs[1] size (batch 256): properties that do not need the (slow) CPU oracle at this size --
    (1) inference is per-image: the first 8 images of the batch give the same posteriors when run alone at batch 8
        (fp32: to fp32 round-off; bf16s: to bf16 round-off, different tiles round the same sums differently) and, in
        fp32, the same greedy indices;
    (2) the greedy decode equals arg-max / collapse-repeats / drop-blank applied to the device posteriors (bit-exact);
    (3) the posteriors are normalised, the per-sample CTC loss is finite and positive, the train step is deterministic."""
    cfg = M.Config()
    B = 256
    p, bn = M.init_params(cfg, seed=2, dtype=np.float32)
    p = M.randomize_params(cfg, p)
    x, lab, il, ll = M.synthetic_batch(cfg, B, seed=9)
    big = Engine(B, dropout=True, precision=precision); big.set_params(p, bn)
    yb = big.forward(x, train=False).clone()
    small = Engine(8, dropout=True, precision=precision); small.set_params(p, bn)
    ys = small.forward(x[:8], train=False)
    tol = 2e-5 if precision == "fp32" else 3e-2
    assert float((yb[:8] - ys).abs().max()) < tol
    gb, lb = big.greedy_decode(yb); gs, ls = small.greedy_decode(ys)
    if precision == "fp32":
        assert torch.equal(gb[:8], gs) and torch.equal(lb[:8], ls)
    yh = yb.cpu().numpy()
    ref, rl = ctc.ctc_greedy_decode(yh, np.full(B, yh.shape[1]))
    assert np.array_equal(gb.cpu().numpy(), ref) and np.array_equal(lb.cpu().numpy(), rl)
    assert np.abs(yh.sum(-1) - 1).max() < 1e-5
    big.forward(x, train=True, seed=4); l1 = big.backward(lab, il, ll, seed=4).clone(); g1 = big.grads.clone()
    big.forward(x, train=True, seed=4); l2 = big.backward(lab, il, ll, seed=4)
    assert torch.equal(l1, l2) and torch.equal(g1, big.grads)
    lh = l1.cpu().numpy()
    assert np.isfinite(lh).all() and (lh > 0).all() and np.isfinite(g1.cpu().numpy()).all()


def test_bf16s_gru_variant_tracks_the_fp32_oracle():
    """The GRU recurrence (what the reference's train.py builds) in the throughput mode: recurrent products on the bf16
    MFMA from bf16 U copies.  Same acceptance as the LSTM variant: forward within bf16 round-off, gradients of the upper
    layers pointing the same way as the fp64 oracle's."""
    cfg = M.Config(gru=True)
    B = 8
    p, bn = M.init_params(cfg, seed=17, dtype=np.float64)
    p = M.randomize_params(cfg, p)
    x, lab, il, ll = M.synthetic_batch(cfg, B, seed=3, dtype=np.float64)
    eng = Engine(B, dropout=False, precision="bf16s", gru=True)
    eng.set_params(p, bn)
    yd = eng.forward(x.astype(np.float32), train=True, seed=0).cpu().numpy()
    loss_d = eng.backward(lab, il, ll, seed=0).cpu().numpy()
    gd = eng.get_grads()
    loss, loss_b, g, c = M.loss_and_grads(cfg, p, bn, x, lab, il, ll)
    agree = (np.argmax(yd, -1) == np.argmax(c["y_pred"], -1)).mean()
    rel_loss = np.abs(loss_d - loss_b).max() / np.abs(loss_b).max()
    cos = {k: float((gd[k].ravel() @ g[k].ravel()) / (np.linalg.norm(gd[k]) * np.linalg.norm(g[k]) + 1e-30)) for k in p if g[k].size >= 512}
    print("[bf16s gru] max|dy|=%.3e agreement=%.4f rel loss err=%.3e" % (np.abs(yd - c["y_pred"]).max(), agree, rel_loss),
          " ".join("%s:%.3f" % kv for kv in cos.items() if kv[0].startswith(("rnn", "dense"))))
    assert np.abs(yd - c["y_pred"]).max() < 5e-2 and agree > 0.93 and rel_loss < 2e-2
    for k in ("dense2_w", "rnn2f_w", "rnn2b_u", "rnn1f_u", "rnn1f_w", "dense1_w"):
        assert cos[k] > 0.95, (k, cos[k])


def test_c_train_step_driver_equals_the_staged_python_step():
    """crnn_train_step_adam (forward -> backward -> clip -> Adam -> BN moving statistics in one C call) must leave exactly
    the state Engine.train_step leaves when it chains the same entry points from Python."""
    import math
    from crnn_mi355x.engine import _ptr, _stream
    from crnn_mi355x.native import check
    from crnn_mi355x.optimizers import Adam
    cfg = M.Config()
    B = 4
    p, bn = M.init_params(cfg, seed=5, dtype=np.float32)
    p = M.randomize_params(cfg, p)
    x, lab, il, ll = M.synthetic_batch(cfg, B, seed=6)
    a = Engine(B, dropout=True, precision="fp32"); a.set_params(p, bn)
    b = Engine(B, dropout=True, precision="fp32"); b.set_params(p, bn)
    opt = Adam(lr=1e-4, beta_1=0.5, beta_2=0.999, clipnorm=5)
    la = a.train_step(x, lab, il, ll, opt, iteration=0, seed=3).clone()
    xd = b._as_input(x); labd, ild, lld = b._as_i32(lab), b._as_i32(il), b._as_i32(ll)
    mom, vel = torch.zeros_like(b.params), torch.zeros_like(b.params)
    lr_t = 1e-4 * math.sqrt(1.0 - 0.999) / (1.0 - 0.5)
    check(b.lib.crnn_train_step_adam(b._c, _ptr(b.params), _ptr(b.grads), _ptr(mom), _ptr(vel), _ptr(b.bn_mean), _ptr(b.bn_var), _ptr(xd),
                                     _ptr(labd), _ptr(ild), _ptr(lld), _ptr(b.ws), b.ws_bytes, _ptr(b.y_pred), _ptr(b.loss),
                                     _ptr(b.norm_scratch), _ptr(b.norm), lr_t, 0.5, 0.999, 1e-7, 5.0, 3, _stream()), "train_step_adam")
    assert torch.equal(la, b.loss) and torch.equal(a.params, b.params)
    assert torch.equal(a.bn_mean, b.bn_mean) and torch.equal(a.bn_var, b.bn_var)
    assert torch.equal(a.opt_state["m"], mom) and torch.equal(a.opt_state["v"], vel)


def test_side_stream_weight_gradients_equal_the_serial_schedule():
    """The backward with a second stream (weight-gradient GEMMs of dense2 / the upper recurrent layer overlapping the BPTT chains,
    crnn_backward_top_ex; the pointwise weight-gradient GEMM of every conv block next to the block's other kernels, gradient
    buffers rotating over three allocations, crnn_backward_bottom_ex) must be bit-identical to the serial schedule, LSTM and GRU,
    fp32 and bf16s, repeated (the rotation and the event reuse must hold from step to step)."""
    for gru in (False, True):
        cfg = M.Config(gru=gru)
        B = 8
        p, bn = M.init_params(cfg, seed=21, dtype=np.float32)
        p = M.randomize_params(cfg, p)
        x, lab, il, ll = M.synthetic_batch(cfg, B, seed=22)
        for precision in ("fp32", "bf16s"):
            eng = Engine(B, dropout=True, precision=precision, gru=gru)
            eng.set_params(p, bn)
            res = {}
            for overlap in (False, True):
                eng.overlap_rnn_wgrad = overlap; eng.overlap_conv_wgrad = overlap
                eng.grads.fill_(float("nan"))
                eng.forward(x, train=True, seed=2)
                loss = eng.backward(lab, il, ll, seed=2).clone()
                torch.cuda.synchronize()
                res[overlap] = (loss, eng.grads.clone())
            assert torch.equal(res[False][0], res[True][0])
            assert torch.equal(res[False][1], res[True][1]), (gru, precision)
            assert torch.isfinite(res[True][1]).all()
            for rep in range(3):                                # again, back to back
                eng.grads.fill_(float("nan"))
                eng.forward(x, train=True, seed=2)
                eng.backward(lab, il, ll, seed=2)
            torch.cuda.synchronize()
            assert torch.equal(res[False][1], eng.grads), (gru, precision, "repeat")


def test_staged_host_batches_train_like_device_resident_ones():
    """Engine.stage (page-locked double-buffered H->D staging of Readf's float64 / int64 host batches, the path Model.fit_generator
    takes, train.py:201-209): three train steps fed through it leave bit-identical weights to the same steps on device-resident tensors,
    including a non-finite row of a short tail batch being zeroed the same way."""
    from crnn_mi355x.init import initial_parameters
    from crnn_mi355x.optimizers import Adam
    cfg = M.Config(imgh=40, max_len=6, time_dense_size=32, n_units=64)
    B = 8
    engs = []
    for _ in range(2):
        e = Engine(B, 40, 32, 38, 6, 32, 64, dropout=True)
        e.set_params(initial_parameters(e.layout, 64, False, seed=5))
        engs.append(e)
    opts = [Adam(lr=1e-3, beta_1=0.5, clipnorm=5), Adam(lr=1e-3, beta_1=0.5, clipnorm=5)]
    X = np.empty((B, 40, 32, 1))                       # the generator's own array, rewritten between steps
    for it in range(3):
        x, lab, il, ll = M.synthetic_batch(cfg, B, seed=20 + it, dtype=np.float64)
        X[...] = x
        if it == 1:
            X[B - 1] = np.nan                          # undefined rows of Readf's tail batch
        sb = engs[0].stage(X, lab, il.reshape(-1, 1), ll.reshape(-1, 1))
        X[...] = -7.0                                  # the generator moves on before the step runs
        engs[0].train_step(sb, None, None, None, opts[0], it)
        xr = x.astype(np.float32)
        if it == 1:
            xr[B - 1] = 0.0
        engs[1].train_step(torch.from_numpy(xr).cuda(), lab, il, ll, opts[1], it)
    torch.cuda.synchronize()
    assert torch.equal(engs[0].params, engs[1].params) and torch.equal(engs[0].bn_mean, engs[1].bn_mean)
    assert torch.equal(engs[0].loss, engs[1].loss)


def test_stn_callable_matches_the_oracle_locnet_and_sampler():
    """utils.STN(image, sampling_size) (utils.py:247-258) as a callable: localisation net + sampler through the C ABI against the oracle
    ops, with given weights; with the reference's initial weights (dense_2 kernel zero, identity bias) it is the identity-theta sampler."""
    from crnn_mi355x.surface import STN, BilinearInterpolation, get_initial_weights
    rs = np.random.RandomState(3)
    B, H, W = 3, 100, 32
    x = rs.normal(size=(B, H, W, 1))
    F = ((H // 2 - 4) // 2 - 4) * ((W // 2 - 4) // 2 - 4) * 20
    ws = [rs.normal(size=(5, 5, 1, 20)) * 0.2, rs.normal(size=20) * 0.1, rs.normal(size=(5, 5, 20, 20)) * 0.05, rs.normal(size=20) * 0.1,
          rs.normal(size=(F, 50)) * 0.05, rs.normal(size=50) * 0.1, rs.normal(size=(50, 6)) * 0.02, np.array([1, 0, 0, 0, 1, 0], np.float64)]
    out = STN(x, (H, W), weights=ws)
    p1 = ops.maxpool_fwd(x, 2, 2)
    c1 = ops.conv_valid_fwd(p1, ws[0], ws[1])
    c2 = ops.conv_valid_fwd(ops.maxpool_fwd(c1, 2, 2), ws[2], ws[3])
    fc1 = ops.relu_fwd(ops.dense_fwd(c2.reshape(B, -1), ws[4], ws[5]))
    theta = ops.dense_fwd(fc1, ws[6], ws[7])
    ref = ops.sampler_fwd(x, theta)
    # (the sampler truncates its source coordinates, utils.py:166-169: a coordinate within fp32 round-off of an integer may pick the
    # neighbouring corner on one side only -- isolated pixels, so the bound is on all but a vanishing fraction of them)
    close = np.abs(out - ref) < 1e-3 * max(1.0, np.abs(ref).max())
    assert out.shape == (B, H, W, 1) and close.mean() > 0.998, close.mean()
    ident = STN(x, (H, W))                              # fresh layers: theta = identity
    same = BilinearInterpolation((H, W))([x, np.tile(get_initial_weights(50)[1], (B, 1))])
    assert np.array_equal(ident, same)
