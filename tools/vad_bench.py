#!/usr/bin/env python3
"""Voice activity detection (conformer_amd.vad, Transcriber(vad=...)): what it costs and what it saves.  Run once; no
threshold is asserted.

Device events after warm-up, best of the alternated passes:
  offline     one recording of --frames mel frames x 80 bins: energy_us (the one cfm3_vad_energy_f32 launch, with the GB/s of
              the mel bytes it reads; energy_cold_us: five single launches, each after 512 MiB were written, so that the
              recording comes from HBM and not from the Infinity Cache), scan_us (the cfm3_vad_scan_f32 launches, one per 4096
              frames) and step_us (StreamingVad.step whole)
  streaming   --slots slots x --chunk mel frames per step: energy_us, scan_us, step_us, beside frontend_step_us, the
              StreamingAudioFrontend.step that makes such a chunk
  longform    Transcriber.transcribe (Conformer-L, beam W=100, 30 s windows, 8 s overlap) on a synthetic log-mel recording of
              --minutes minutes, every other 10 s at the low level: the windows encoded and the wall time with vad off and on."""
import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conformer_amd import _lib, ops  # noqa: E402
from conformer_amd.vad import SCAN_FRAMES, StreamingVad, VadConfig  # noqa: E402

CONFIG = VadConfig(snr_db=9.0)


def timed(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def synthetic(S, n_mel, T, dev, period=1000):
    """log-mel frames: Gaussian around -6, every other `period` frames 6 nats louder but for a pause of 10 frames in every 100
    (shorter than the hangover; without pauses the noise floor would rise to the level of the speech after noise_window)"""
    x = torch.randn(S, n_mel, T, device=dev) - 6.0
    t = torch.arange(T, device=dev)
    loud = ((t // period) % 2 == 1) & (t % 100 >= 10)
    return x + 6.0 * loud


def detector(S, T, iters, dev):
    vad = StreamingVad(S, 80, CONFIG, 0.01, max_segments=max(64, T // 35 + 1), device=dev)
    x = synthetic(S, 80, T, dev)
    k = torch.full((S,), T, dtype=torch.int64, device=dev)
    vad.step(x, k)
    p, stream = vad.p, ops._stream()
    ks = [(t0, min(SCAN_FRAMES, T - t0), (k - t0).clamp(0, min(SCAN_FRAMES, T - t0))) for t0 in range(0, T, SCAN_FRAMES)]

    def scan():
        for t0, n, kk in ks:
            _lib.call("cfm3_vad_scan_f32", vad.energy.data_ptr() + 4 * t0, T, kk.data_ptr(), n, p.smooth, p.noise_window, p.snr,
                      p.min_energy, p.onset, p.hangover, vad.state.data_ptr(), vad.ring.data_ptr(), vad.flags.data_ptr() + t0, T,
                      vad.segments.data_ptr(), vad.max_segments, S, stream)

    fns = {
        "energy": lambda: _lib.call("cfm3_vad_energy_f32", x.data_ptr(), 80 * T, T, k.data_ptr(), T, 80, 0, 80,
                                    vad.energy.data_ptr(), T, S, stream),
        "scan": scan,
        "step": lambda: vad.step(x, k),
    }
    res = {"slots": S, "mel_frames": T, "mel_bytes": 4 * S * 80 * T, "scan_launches": len(ks)}
    for _ in range(2):
        for name, fn in fns.items():
            us = timed(fn, iters)
            res[name + "_us"] = min(res.get(name + "_us", us), us)
    res["energy_GBps"] = res["mel_bytes"] / res["energy_us"] * 1e-3
    if res["mel_bytes"] >= 1 << 26:
        # back-to-back launches find a recording below 256 MiB in the Infinity Cache; from HBM: 512 MiB written in between
        flush = torch.empty(1 << 27, dtype=torch.float32, device=dev)
        cold = []
        for _ in range(5):
            flush.fill_(1.0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fns["energy"]()
            e1.record()
            torch.cuda.synchronize()
            cold.append(e0.elapsed_time(e1) * 1e3)
        res["energy_cold_us"] = sorted(cold)
        res["energy_cold_GBps"] = res["mel_bytes"] / sorted(cold)[2] * 1e-3          # (the median)
    return res


def front_end(S, chunk, iters, dev):
    from conformer_amd.frontend import ConformerAudioFrontend
    from conformer_amd.stream_frontend import StreamingAudioFrontend
    base = ConformerAudioFrontend(device=dev)
    n = chunk * base.hop_length
    fe = StreamingAudioFrontend(base, S, n)
    for s in range(S):
        fe.open(s)
    x = 0.3 * torch.randn(S, n, device=dev)
    fe.step(x, [n] * S)
    return min(timed(lambda: fe.step(x, [n] * S), iters) for _ in range(2))


def longform(minutes, dev):
    from conformer_amd.decode import BeamCTCDecoder
    from conformer_amd.longform import BufferedEncoder, Transcriber
    from model.conformer import Conformer
    vocab = ["<pad>"] + [chr(ord("a") + i) for i in range(26)] + ["'", "|", "<unk>"]
    m = Conformer(len(vocab), 80, 16, 512, 8, 31, 640, 1, 0.0).to(dev).eval()
    dec = BeamCTCDecoder(vocab, blank_id=0, skip_ids=(len(vocab) - 1,), beam_width=100)
    x = synthetic(1, 80, int(minutes * 6000), dev)[0]
    res = {"mel_frames": x.shape[1]}
    plan, planned = BufferedEncoder.plan, []
    BufferedEncoder.plan = lambda self, n: planned.append(plan(self, n)) or planned[-1]
    try:
        for name, cfg in (("off", None), ("on", CONFIG)):
            tr = Transcriber(m, dec, window_seconds=30.0, overlap_seconds=8.0, vad=cfg)
            tr.transcribe([x])                                               # packs, tables
            best = math.inf
            for _ in range(2):
                del planned[:]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = tr.transcribe([x])
                torch.cuda.synchronize()
                best = min(best, time.perf_counter() - t0)
            res[f"vad_{name}"] = {"windows": sum(len(ws) for ws in planned[-1]), "frames_decoded": out[0].frames,
                                  "wall_ms": best * 1e3}
            if cfg is not None:
                res["islands"] = len(tr.speech([x])[0])
    finally:
        BufferedEncoder.plan = plan
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=360000, help="mel frames of the offline recording (one hour at 10 ms)")
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--chunk", type=int, default=64, help="mel frames per slot and streaming step")
    ap.add_argument("--minutes", type=float, default=10.0, help="length of the long-form recording")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-longform", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    _lib.check(_lib.load().cfm_device_check(), "cfm_device_check")
    torch.manual_seed(0)
    out = {"what": "voice activity detection: the energy and scan launches offline and per streaming step, and "
                   "Transcriber.transcribe with vad off and on"}
    with torch.no_grad():
        out["offline"] = detector(1, args.frames, args.iters, dev)
        print(json.dumps(out["offline"]), file=sys.stderr, flush=True)
        out["streaming"] = detector(args.slots, args.chunk, args.iters * 5, dev)
        out["streaming"]["frontend_step_us"] = front_end(args.slots, args.chunk, args.iters * 5, dev)
        print(json.dumps(out["streaming"]), file=sys.stderr, flush=True)
        if not args.no_longform:
            out["longform"] = longform(args.minutes, dev)
            print(json.dumps(out["longform"]), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
