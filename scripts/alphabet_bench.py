#!/usr/bin/env python3
"""The three timings DESIGN.md quotes for the class count, at a chosen alphabet (38: one class per lane in the softmax / CTC / beam kernels; 65..128: two):
the crnn_ctc_loss_grad launch at batch 256 (as scripts/ctc_bench.py), the bf16s training step at batch 256 (as bench.py's headline) and forward + beam search
(beam_width 10) at batch 1024 (as bench.predict_leg).  Prints one JSON line.  usage: alphabet_bench.py [--classes 97] [--steps 20] [--warmup 5]"""
import argparse, ctypes, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "crnn-ocr-lite_amd")]
import numpy as np
import torch
from bench import synthetic_batch, timed_steps
from crnn_mi355x import native
from crnn_mi355x.engine import Engine
from crnn_mi355x.init import initial_parameters
from crnn_mi355x.optimizers import Adam

ap = argparse.ArgumentParser()
ap.add_argument("--classes", type=int, default=97)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--iters", type=int, default=20)
args = ap.parse_args()
C = args.classes
P = lambda t: ctypes.c_void_p(t.data_ptr())
S = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def events(fn, n, warm):
    ts = []
    for it in range(warm + n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        if it >= warm:
            ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def dev_batch(B, T):
    x, lab, il, ll = synthetic_batch(B, seed=0, num_classes=C, T=T)
    i32 = lambda a: torch.from_numpy(a.astype(np.int32)).cuda()
    return torch.from_numpy(x).cuda(), i32(lab), i32(il), i32(ll)


out = {"classes": C, "classes_per_lane": 1 if C <= 64 else 2}
# ---- the CTC launch
B, T, Lmax = 256, 52, 23
_, labd, ild, lld = dev_batch(B, T)
y = torch.softmax(torch.randn(B, T, C, device="cuda") * 2, -1).contiguous()
loss = torch.zeros(B, device="cuda"); dl = torch.zeros(T, B, C, device="cuda")
lib = native.lib()


def ctc_launch():
    rc = lib.crnn_ctc_loss_grad(P(y), P(labd), P(ild), P(lld), P(loss), P(dl), B, T, C, Lmax, 2, ctypes.c_float(1.0 / B), S())
    assert rc == 0, rc
out["ctc_loss_grad_us_batch256"] = round(1e3 * events(ctc_launch, 30, 5), 1)     # (incl. ~2 us of event latency)
# ---- the training step
eng = Engine(B, num_classes=C, dropout=True, precision="bf16s")
eng.set_params(initial_parameters(eng.layout, eng.cfg.units, False, seed=1))
dt, last = timed_steps(eng, dev_batch(B, eng.T), Adam(lr=1e-4, beta_1=0.5, beta_2=0.999, clipnorm=5), args.steps, args.warmup)
_, giveups = eng.loss_and_status().tolist()
eng.raise_if_rnn_gave_up(giveups)
out.update({"train_ms_per_step_batch256": round(1e3 * dt / args.steps, 3), "train_images_per_sec": round(B * args.steps / dt, 1), "final_loss": round(last, 4)})
del eng
torch.cuda.empty_cache()
# ---- forward + beam search
B = 1024
eng = Engine(B, num_classes=C, dropout=False, precision="bf16s")
p = initial_parameters(eng.layout, eng.cfg.units, False, seed=1)
rs = np.random.RandomState(2)
for k in p:                                        # non-degenerate posteriors, as bench.predict_leg draws them
    if k.endswith(("_b", "_g")) or k == "stn_d2_w":
        p[k] = (p[k] + rs.normal(size=p[k].shape) * (0.02 if k.startswith("stn_d2") else 0.3)).astype(np.float32)
eng.set_params(p)
xd = dev_batch(B, eng.T)[0]
state = {}


def both():
    state["y"] = eng.forward(xd, train=False)
    state["beam"] = eng.beam_decode(state["y"], beam_width=10)
t50 = events(both, args.iters, 3)
b50 = events(lambda: eng.beam_decode(state["y"], beam_width=10), args.iters, 0)
eng.check_rnn_status()
lab = state["beam"][0]
out.update({"forward_plus_beam_ms_p50_batch1024": round(t50, 3), "beam_decode_ms_p50_batch1024": round(b50, 3),
            "latency_us_per_image_p50": round(1e3 * t50 / B, 3), "decoded_ids_at_or_above_64": int((lab >= 64).sum().item())})
print(json.dumps(out), flush=True)
