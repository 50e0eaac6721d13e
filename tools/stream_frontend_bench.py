#!/usr/bin/env python3
"""Streaming audio front end (conformer_amd.stream_frontend.StreamingAudioFrontend): S slots, every slot fed the same number of
samples per step, mid-stream (every slot carries a tail, no flush).

Per (S, samples per step), device events after warm-up, best of two alternated passes:
  step_us      StreamingAudioFrontend.step whole (table copy, staging, DFT GEMM, power + mel + log)
  stage_us, dft_us, mel_us   the three launches of that step on their own, on the step's own buffers
  offline_us   one ConformerAudioFrontend.mel_spectrogram over the same (S, samples) audio
and, unless --no-transcriber, beside them
  transcriber_step_ms   SlotTranscriber.step (Conformer-L, beam W=100, no LM) on the mel chunk those samples make, host clock
                        around a synchronise, median
A fused stage + DFT + mel kernel would have to beat stage_us + dft_us + mel_us; what the front end adds to a service's step is
step_us against transcriber_step_ms."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conformer_amd import _lib, ops  # noqa: E402
from conformer_amd.frontend import ConformerAudioFrontend  # noqa: E402
from conformer_amd.stream_frontend import StreamingAudioFrontend  # noqa: E402


def timed(fn, iters, warm=5):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def front_end(S, n, iters, dev):
    base = ConformerAudioFrontend(device=dev)
    fe = StreamingAudioFrontend(base, S, n)
    for s in range(S):
        fe.open(s)
    x = 0.3 * torch.randn(S, n, device=dev)
    counts = [n] * S
    mel, frames = fe.step(x, counts)                                      # from here on every slot is mid-stream
    mel, frames = fe.step(x, counts)
    f_max, hop, n_fft = max(frames), fe.hop, fe.n_fft
    rpu, nb2, stream = f_max + fe.extra, base.basis.shape[0], ops._stream()
    fns = {
        "step": lambda: fe.step(x, counts),
        # the launches of the last step again (same table; the tail it reads is the next step's: the same amount of work)
        "stage": lambda: _lib.call("cfm_stream_stage_f32", x.data_ptr(), n, n, fe.tails[0].data_ptr(), fe.tails[1].data_ptr(),
                                   fe.table.data_ptr(), fe.xp.data_ptr(), S, f_max, hop, n_fft, stream),
        "dft": lambda: _lib.call("cfm_dft_frames_f32", fe.xp.data_ptr(), base.basis.data_ptr(), fe.spec.data_ptr(), S * rpu, nb2,
                                 n_fft, hop, stream),
        "mel": lambda: _lib.call("cfm_power_mel_log_mfma_f32", fe.spec.data_ptr(), nb2, base.fbT.data_ptr(), mel.data_ptr(), S,
                                 f_max, rpu, n_fft // 2 + 1, base.n_mels, 1e-5, stream),
        "offline": lambda: base.mel_spectrogram(x),
    }
    res = {"slots": S, "samples_per_step": n, "mel_frames_per_step": f_max}
    for _ in range(2):
        for name, fn in fns.items():
            us = timed(fn, iters)
            res[name + "_us"] = min(res.get(name + "_us", us), us)
    res["stage_bytes"] = 4 * (S * n + S * rpu * hop + n_fft + 2 * S * 512)   # samples read, xp written, tails read and written
    res["stage_GBps"] = res["stage_bytes"] / res["stage_us"] * 1e-3
    return res


def transcriber(m, dec, S, mel_frames, steps, dev):
    from conformer_amd.slots import SlotTranscriber
    x = torch.randn(S, 80, mel_frames, device=dev)
    best = None
    for _ in range(2):                                                     # the first pass warms up (packs, tables)
        tr = SlotTranscriber(m, dec, S, mel_frames * (steps + 1))
        for s in range(S):
            tr.open(s)
        lat = []
        torch.cuda.synchronize()
        for _ in range(steps):
            t0 = time.perf_counter()
            tr.step(x, [mel_frames] * S)
            torch.cuda.synchronize()
            lat.append((time.perf_counter() - t0) * 1e3)
        del tr
        torch.cuda.empty_cache()
        med = sorted(lat[1:])[len(lat[1:]) // 2]
        best = med if best is None else min(best, med)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--samples", type=int, nargs="+", default=[10240, 102400], help="samples per slot and step")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--transcriber-steps", type=int, default=6)
    ap.add_argument("--no-transcriber", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    _lib.check(_lib.load().cfm_device_check(), "cfm_device_check")
    torch.manual_seed(0)
    out = {"what": "streaming audio front end: per-step time by launch, beside SlotTranscriber.step and the offline front end",
           "runs": []}
    m = dec = None
    if not args.no_transcriber:
        from conformer_amd.decode import BeamCTCDecoder
        from model.conformer import Conformer
        vocab = ["<pad>"] + [chr(ord("a") + i) for i in range(26)] + ["'", "|", "<unk>"]
        m = Conformer(len(vocab), 80, 16, 512, 8, 31, 640, 1, 0.0).to(dev).eval()
        dec = BeamCTCDecoder(vocab, blank_id=0, skip_ids=(len(vocab) - 1,), beam_width=100)
    with torch.no_grad():
        for S in args.slots:
            for n in args.samples:
                run = front_end(S, n, args.iters, dev)
                if m is not None:
                    run["transcriber_step_ms"] = transcriber(m, dec, S, run["mel_frames_per_step"], args.transcriber_steps, dev)
                    run["front_end_share_of_step"] = run["step_us"] * 1e-3 / (run["step_us"] * 1e-3 + run["transcriber_step_ms"])
                out["runs"].append(run)
                print(json.dumps(run), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
