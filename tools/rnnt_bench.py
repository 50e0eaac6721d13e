#!/usr/bin/env python3
"""The transducer (conformer_amd.ops.rnnt_*, ConformerCriterion.rnnt_loss, model/transducer.py, decode.rnnt_greedy_decode): what
the loss, the joint's combine, a whole training step and the greedy decode cost.  Run once; no threshold is asserted.  Writes --out
(profiles/rnnt_bench.json) and prints the same JSON.

Device events after warm-up, best of the alternated passes, at B = --batch (32), T' = --frames (249), U1 = --labels + 1 (51),
J = --joint (640), ragged lengths, for V in {370, 4096}:
  loss_fwd          cfm3_rnnt_loss_fwd_f32 (workspace allocation included): the row pass and the two lattices
  loss_fwd_bwd      ... followed by cfm3_rnnt_loss_bwd_f32: the second row pass, dlogits (B, T', U1, V)
  lattice           loss_fwd at V = 4 and the same lengths, where the row pass moves 1 % of the V = 370 bytes: the latency chain
  rows_fwd / rows_bwd   loss_fwd - lattice and loss_fwd_bwd - loss_fwd: the two V-wide passes, with the bytes each moves by
                    construction (live rows read, every row of dlogits written) and bytes / time as a fraction of the HBM peak
                    (8 TB/s; about 6.3 TB/s is achievable with plain streaming).  Both times are DIFFERENCES of two timings, not
                    kernel times: the V = 4 run that is subtracted holds a row kernel, a launch and the workspace allocation of its
                    own, so rows_fwd is under-stated by that much and its share of the peak is an upper bound
  joint_fwd / joint_bwd cfm3_rnnt_joint_fwd_f32 and _bwd_f32 alone, measured the same way (h written once; h and dh read twice)
  logits_bytes, peak_bytes   the (B, T', U1, V) block, and the peak allocation over loss forward + backward beyond the logits
The whole step: ConformerTransducer at the flagship encoder (16 blocks, d 256) on B x --seconds (10 s) of 80-mel features, forward,
rnnt_loss and backward, beside Conformer forward, ctc_loss and backward on the same input: time and peak memory of each.
Greedy decode of the same B x 10 s with untrained weights, at the output bias as drawn (every frame then runs into the cap of
max_symbols = 10: the worst case) and with the blank's bias raised by 1 (blank then wins nearly everywhere: the best case): tokens, iterations, C-ABI
calls per iteration, host time to the result for sync_every in {4, 16, 64}."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from conformer_amd import _lib, decode, ops  # noqa: E402
from conformer_amd.evaluation import ConformerCriterion  # noqa: E402

HBM_PEAK, HBM_STREAM = 8.0e12, 6.3e12


def timed(fn, iters, warm=2):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def best(fns, iters):
    res = {}
    for _ in range(2):
        for name, fn in fns.items():
            us = timed(fn, iters)
            res[name + "_us"] = round(min(res.get(name + "_us", us), us), 1)
    return res


def lengths(B, T, U, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    in_len = torch.randint(max(1, T - 40), T + 1, (B,), generator=g)
    tg_len = torch.randint(max(0, U - 8), U + 1, (B,), generator=g)
    in_len[0], tg_len[0] = T, U
    return in_len.to(dev), tg_len.to(dev)


def share(nbytes, us):
    rate = nbytes / (us * 1e-6)
    return {"bytes": int(nbytes), "us": round(us, 1), "TB_per_s": round(rate / 1e12, 3), "of_hbm_peak": round(rate / HBM_PEAK, 3),
            "of_hbm_streaming": round(rate / HBM_STREAM, 3)}


def loss_shape(B, T, U1, V, dev, iters):
    g = torch.Generator().manual_seed(V)
    in_len, tg_len = lengths(B, T, U1 - 1, dev)
    targets = torch.randint(1, V, (B, U1 - 1), generator=g).to(dev)
    x = torch.randn(B, T, U1, V, device=dev)
    x4 = torch.randn(B, T, U1, 4, device=dev)
    w = torch.randn(B, device=dev)

    def fwd():
        return ops.rnnt_loss_forward(x, targets, in_len, tg_len, 0)

    def fwd_bwd():
        _, ctx = ops.rnnt_loss_forward(x, targets, in_len, tg_len, 0)
        return ops.rnnt_loss_backward(ctx, w)

    def lattice():
        return ops.rnnt_loss_forward(x4, targets.clamp_max(3), in_len, tg_len, 0)

    res = dict(B=B, T=T, U1=U1, V=V)
    res.update(best({"loss_fwd": fwd, "loss_fwd_bwd": fwd_bwd, "lattice": lattice}, iters))
    live = int(((in_len) * (tg_len + 1)).sum())
    cells = B * T * U1
    res["live_rows"], res["rows"] = live, cells
    # differences of two timings (see the module docstring): not kernel times
    res["rows_fwd"] = share(live * V * 4 + 3 * live * 4, max(res["loss_fwd_us"] - res["lattice_us"], 1e-3))
    res["rows_bwd"] = share(live * V * 4 + cells * V * 4 + live * (3 * 4 + 3 * 8), max(res["loss_fwd_bwd_us"] - res["loss_fwd_us"], 1e-3))
    res["rows_fwd"]["how"] = "loss_fwd_us - lattice_us (a V = 4 run): an upper bound on the rate"
    res["rows_bwd"]["how"] = "loss_fwd_bwd_us - loss_fwd_us"
    res["logits_bytes"] = cells * V * 4
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fwd_bwd()
    torch.cuda.synchronize()
    res["peak_bytes_beyond_inputs"] = torch.cuda.max_memory_allocated() - before
    return res


def joint_shape(B, T, U1, J, dev, iters):
    e, p = torch.randn(B, T, J, device=dev), torch.randn(B, U1, J, device=dev)
    h = ops.rnnt_joint_forward(e, p)
    dh = torch.randn(B, T, U1, J, device=dev)
    res = dict(B=B, T=T, U1=U1, J=J)
    t = best({"joint_fwd": lambda: ops.rnnt_joint_forward(e, p), "joint_bwd": lambda: ops.rnnt_joint_backward(h, dh)}, iters)
    block = B * T * U1 * J * 4
    res["joint_fwd"] = share(block + (B * T + B * U1) * J * 4, t["joint_fwd_us"])
    res["joint_bwd"] = share(4 * block + (B * T + B * U1) * J * 4, t["joint_bwd_us"])
    return res


def features(B, seconds, dev):
    g = torch.Generator().manual_seed(1)
    T = int(seconds * 100)
    feats = torch.randn(B, 80, T, generator=g).to(dev)
    lens = torch.randint(T - 160, T + 1, (B,), generator=g)
    lens[0] = T
    return feats, lens.to(dev)


def whole_step(B, seconds, U, V, dev, iters):
    from model.conformer import Conformer
    from model.transducer import ConformerTransducer
    feats, lens = features(B, seconds, dev)
    g = torch.Generator().manual_seed(2)
    targets = torch.randint(1, V, (B, U), generator=g).to(dev)
    _, tg_len = lengths(B, 8, U, dev)
    crit = ConformerCriterion(0)
    res = dict(B=B, seconds=seconds, U1=U + 1, V=V)
    for name in ("transducer", "ctc"):
        torch.manual_seed(3)
        if name == "transducer":
            m = ConformerTransducer(V).to(dev).train()

            def step():
                m.zero_grad(set_to_none=True)
                logits, out_len = m(feats, lens, targets, tg_len)
                crit.rnnt_loss(logits, targets, out_len, tg_len).backward()
        else:
            m = Conformer(V).to(dev).train()

            def step():
                m.zero_grad(set_to_none=True)
                logits, out_len = m(feats, lens)
                crit.ctc_loss(logits, targets, out_len, tg_len).backward()
        res[name + "_step_us"] = round(min(timed(step, iters, warm=2), timed(step, iters, warm=0)), 1)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        step()
        torch.cuda.synchronize()
        res[name + "_peak_bytes"] = torch.cuda.max_memory_allocated()
        del m
        torch.cuda.empty_cache()
    res["transducer_over_ctc_time"] = round(res["transducer_step_us"] / res["ctc_step_us"], 3)
    return res


def greedy(B, seconds, V, dev, max_symbols=10):
    from model.transducer import ConformerTransducer
    torch.manual_seed(4)
    m = ConformerTransducer(V).to(dev).eval()
    feats, lens = features(B, seconds, dev)
    with torch.no_grad():
        enc, out_len = m.encoder(feats, lens)
    T = enc.shape[1]

    def calls(fn):
        torch.cuda.synchronize()
        before = _lib.CALLS[0]
        fn()
        return _lib.CALLS[0] - before

    # without a host read the loop runs its T (max_symbols + 1) iterations: two caps give the calls of one iteration
    few = enc[:, :4].contiguous()
    c1 = calls(lambda: decode.rnnt_greedy_decode(m.predictor, m.joiner, few, None, 1, sync_every=1 << 30))
    c2 = calls(lambda: decode.rnnt_greedy_decode(m.predictor, m.joiner, few, None, 2, sync_every=1 << 30))
    per_iter = (c2 - c1) // 4
    setup = c1 - 8 * per_iter
    res = dict(B=B, seconds=seconds, V=V, T=T, max_symbols=max_symbols, abi_calls_per_iteration=per_iter,
               torch_ops_per_iteration="3 (the embedding's clamp and gather, the candidate state's copy)", cases=[])
    for raise_blank in (0.0, 1.0):
        with torch.no_grad():
            m.joiner.out.bias[m.blank_id] += raise_blank
        case = {"blank_bias_raised_by": raise_blank}
        for k in (4, 16, 64):
            times = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n = calls(lambda: decode.rnnt_greedy_decode(m.predictor, m.joiner, enc, out_len, max_symbols, sync_every=k))
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
            case[f"sync_every_{k}_ms"] = round(min(times[1:]) * 1e3, 2)
            case[f"sync_every_{k}_iterations"] = (n - setup) // per_iter
        tokens, counts, _ = decode.rnnt_greedy_decode(m.predictor, m.joiner, enc, out_len, max_symbols)
        case["tokens"] = int(counts.sum())
        case["iteration_cap"] = T * (max_symbols + 1)
        res["cases"].append(case)
    totals = {k: sum(c[f"sync_every_{k}_ms"] for c in res["cases"]) for k in (4, 16, 64)}
    res["sync_every_fastest"] = min(totals, key=totals.get)             # over both cases; decode.RNNT_SYNC_EVERY follows it
    res["sync_every_default"] = decode.RNNT_SYNC_EVERY
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=249)
    ap.add_argument("--labels", type=int, default=50)
    ap.add_argument("--joint", type=int, default=640)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--skip", default="", help="comma list of: loss, joint, step, greedy")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rnnt_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "rnnt_bench needs the MI355X"
    dev = torch.device("cuda:0")
    skip = set(a.skip.split(","))
    out = {"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK, "hbm_streaming_bytes_per_s": HBM_STREAM}
    U1 = a.labels + 1
    if "loss" not in skip:
        out["loss"] = [loss_shape(a.batch, a.frames, U1, V, dev, a.iters) for V in (370, 4096)]
    if "joint" not in skip:
        out["joint"] = joint_shape(a.batch, a.frames, U1, a.joint, dev, a.iters)
    if "step" not in skip:
        out["steps"] = [whole_step(a.batch, a.seconds, a.labels, V, dev, max(2, a.iters // 2)) for V in (370, 4096)]
    if "greedy" not in skip:
        out["greedy"] = greedy(a.batch, a.seconds, 370, dev)
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
