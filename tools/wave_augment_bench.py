#!/usr/bin/env python3
"""Waveform augmentation (conformer_amd.wave_augment) stage by stage at a training batch, 32 rows of 10 s at 16 kHz by default,
beside the log-mel of the same batch.  Run once; no threshold is asserted.  Writes --out (profiles/wave_augment_bench.json) and
prints the same JSON.

Device events after warm-up, best of --passes alternated passes, microseconds per call:
  reverb_K4000 / reverb_K8000   apply with every row reverberated by a response of K taps (the table copy + the FIR launch);
                                GFLOPs = 2 B L K / time, peak_share = that over the 157.3 TF fp32 vector peak
  mix                           apply with every row mixed with noise at a drawn SNR (table copy + powers + mix);
                                GBps = the bytes the two launches must move (x twice, the noise twice, y once) / time
  speed_11_10                   apply with every row at 11:10 (table copy + gather + resampler + scatter)
  whole                         draw + apply with the default speeds, p_reverb = 0.5 at K = 8000, p_noise = 0.7: plans drawn once
                                from a seed and replayed, so every pass times the same work
  mel_spectrogram               the log-mel front end on the same batch"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conformer_amd import _lib  # noqa: E402
from conformer_amd.frontend import ConformerAudioFrontend  # noqa: E402
from conformer_amd.wave_augment import NoiseBank, RirBank, WaveAugment, WavePlan  # noqa: E402

FP32_VECTOR_PEAK = 157.3e12


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


def rir(K, gen):
    """A decaying-noise response of K taps with its direct path 40 samples in."""
    h = torch.randn(K, generator=gen, dtype=torch.float64) * torch.exp(-torch.arange(K, dtype=torch.float64) / (K / 7.0))
    h[40] = 4.0
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "wave_augment_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    _lib.check(_lib.load().cfm_device_check(), "cfm_device_check")
    gen = torch.Generator().manual_seed(0)
    fe = ConformerAudioFrontend(device=dev)
    B, L = a.batch, int(round(fe.sample_rate * a.seconds))
    lengths = [L] * B
    x = (0.3 * torch.randn(B, L, generator=gen)).to(dev)
    noise = NoiseBank([torch.randn(n, generator=gen) for n in (3 * L // 2, L // 3, 50000)])
    rirs = {K: RirBank([rir(K, gen) for _ in range(4)]) for K in (4000, 8000)}
    same = dict(speed=[0] * B, rir=[-1] * B, clip=[-1] * B, offset=[0] * B, snr_db=[15.0] * B, gain_db=[0.0] * B)
    fns, work = {}, {}
    for K, bank in rirs.items():
        wa = WaveAugment(speeds=None, p_reverb=1.0, rirs=bank, device=dev)
        plan = WavePlan(**{**same, "rir": [b % 4 for b in range(B)]})
        fns[f"reverb_K{K}"] = lambda wa=wa, plan=plan: wa.apply(x, lengths, plan)
        work[f"reverb_K{K}"] = 2.0 * B * L * K
    wa_mix = WaveAugment(speeds=None, p_noise=1.0, noise=noise, device=dev)
    plan_mix = WavePlan(**{**same, "clip": [b % 3 for b in range(B)], "offset": [(997 * b) % 50000 for b in range(B)]})
    fns["mix"] = lambda: wa_mix.apply(x, lengths, plan_mix)
    wa_speed = WaveAugment(speeds=((11, 10),), device=dev)
    fns["speed_11_10"] = lambda: wa_speed.apply(x, lengths, WavePlan(**same))
    whole = WaveAugment(p_reverb=0.5, rirs=rirs[8000], p_noise=0.7, noise=noise, snr_db=(5, 25), device=dev)
    whole.generator = torch.Generator().manual_seed(1)
    plans = [whole.draw(lengths) for _ in range(8)]
    turn = [0]

    def run_whole():
        turn[0] += 1
        return whole.apply(x, lengths, plans[turn[0] % len(plans)])

    fns["whole"] = run_whole
    fns["mel_spectrogram"] = lambda: fe.mel_spectrogram(x)
    res = {"what": "waveform augmentation by stage beside the log-mel of the same batch, microseconds per call", "batch": B,
           "samples": L, "iters": a.iters, "passes": a.passes, "us": {}}
    with torch.no_grad():
        for _ in range(a.passes):
            for name, fn in fns.items():
                us = timed(fn, a.iters)
                res["us"][name] = min(res["us"].get(name, us), us)
    for name, flop in work.items():
        rate = flop / (res["us"][name] * 1e-6)
        res[name] = {"GFLOPs": rate * 1e-9, "fp32_vector_peak_share": rate / FP32_VECTOR_PEAK}
    res["mix_GBps"] = 5.0 * 4 * B * L / (res["us"]["mix"] * 1e-6) * 1e-9
    res["whole_plans"] = {"reverb_rows": [sum(r >= 0 for r in p.rir) for p in plans],
                          "noise_rows": [sum(c >= 0 for c in p.clip) for p in plans]}
    res["whole_over_mel"] = res["us"]["whole"] / res["us"]["mel_spectrogram"]
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
