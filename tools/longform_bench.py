#!/usr/bin/env python3
"""Offline long-form transcription (conformer_amd/longform.py): seconds of audio per second, stage by stage.

The BASELINE cfg-2 model (Conformer-L: 16 blocks, d = 512, 8 heads, kernel 31, LSTM 640) with random weights on --minutes of
synthetic 16 kHz audio (one recording each), windows of --window / --overlap seconds in batches of --batch-windows:

  frontend   ConformerAudioFrontend on the whole waveform
  encoder    BufferedEncoder.encode: every window through Encoder.forward, stitched; graphs off and on
  head       model.decoder (LSTM, Swish + BatchNorm, vocabulary Linear) over the stitched frames
  search     BeamCTCDecoder over the logits of the whole recording
  total      Transcriber.transcribe end to end (graphs off and on)
  streaming  the same mel frames through StreamingTranscriber(left_context=...) in --chunk frame steps, for comparison: bounded
             history, no right context, strictly in sequence

Every figure is the best of --repeats passes after one warm-up pass.  No threshold: the file reports what the run gives.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conformer_amd.decode import BeamCTCDecoder  # noqa: E402
from conformer_amd.frontend import ConformerAudioFrontend  # noqa: E402
from conformer_amd.longform import Transcriber, window_plan  # noqa: E402
from conformer_amd.transcribe import StreamingTranscriber  # noqa: E402
from model.conformer import Conformer  # noqa: E402


def best_of(fn, repeats):
    """(best seconds, last result) of fn() over repeats passes after one warm-up pass"""
    best, out = None, None
    for i in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if i and (best is None or dt < best):
            best = dt
    return best, out


def offline(m, dec, fe, wave, args, audio_s):
    res = {}
    tr = {g: Transcriber(m, dec, fe, window_seconds=args.window, overlap_seconds=args.overlap, batch_windows=args.batch_windows,
                         graphs=g) for g in (False, True)}
    t, mels = best_of(lambda: tr[False].features([wave]), args.repeats)
    res["frontend_s"] = t
    n_mel = mels[0].shape[1]
    plan = window_plan(n_mel, tr[False].window, tr[False].overlap)
    res.update(mel_frames=n_mel, window_mel_frames=tr[False].window, overlap_mel_frames=tr[False].overlap, windows=len(plan),
               encoder_frames=plan[-1].keep_to)
    for g in (False, True):
        t, hs = best_of(lambda: tr[g].encoder.encode(mels), args.repeats)
        res["encoder_graphs_s" if g else "encoder_s"] = t
    t, logits = best_of(lambda: tr[False].decoder_head(hs[0][None]), args.repeats)
    res["head_s"] = t
    t, text = best_of(lambda: dec(logits), args.repeats)
    res["search_s"] = t
    del hs, logits
    for g in (False, True):
        t, out = best_of(lambda: tr[g].transcribe([wave]), args.repeats)
        res["total_graphs_s" if g else "total_s"] = t
        res["audio_seconds_per_second_graphs" if g else "audio_seconds_per_second"] = audio_s / t
    res["text_characters"] = len(out[0].text)
    return res, mels[0]


def streaming(m, dec, mel, args, audio_s):
    n = mel.shape[1]
    tr = StreamingTranscriber(m, dec, 1, n, left_context=args.left_context, max_chunk_mel_frames=args.chunk)
    x = mel[None]

    def run():
        tr.reset()
        for t0 in range(0, n, args.chunk):
            tr.step(x[:, :, t0:t0 + args.chunk])
        return tr.finish()

    t, text = best_of(run, args.repeats)
    return {"left_context": args.left_context, "chunk_mel_frames": args.chunk, "total_s": t,
            "audio_seconds_per_second": audio_s / t, "text_characters": len(text[0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, nargs="+", default=[10.0, 60.0])
    ap.add_argument("--window", type=float, default=30.0, help="seconds")
    ap.add_argument("--overlap", type=float, default=8.0, help="seconds")
    ap.add_argument("--batch-windows", type=int, default=32)
    ap.add_argument("--beam", type=int, default=100)
    ap.add_argument("--left-context", type=int, default=256, help="the streaming comparison's history, encoder frames")
    ap.add_argument("--chunk", type=int, default=640, help="the streaming comparison's step, mel frames")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    vocab = ["<pad>"] + [chr(ord("a") + i) for i in range(26)] + ["'", "|", "<unk>"]
    m = Conformer(len(vocab), 80, 16, 512, 8, 31, 640, 1, 0.0).to(dev).eval()
    dec = BeamCTCDecoder(vocab, blank_id=0, skip_ids=(len(vocab) - 1,), beam_width=args.beam)
    fe = ConformerAudioFrontend(device=dev)
    out = {"what": "offline long-form transcription, cfg-2 model, random weights, synthetic audio; seconds, best of repeats",
           "window_seconds": args.window, "overlap_seconds": args.overlap, "batch_windows": args.batch_windows,
           "beam_width": args.beam, "repeats": args.repeats, "runs": []}
    for minutes in args.minutes:
        audio_s = minutes * 60.0
        wave = torch.randn(int(audio_s * fe.sample_rate), device=dev) * 0.1
        res, mel = offline(m, dec, fe, wave, args, audio_s)
        del wave
        run = {"audio_minutes": minutes, "offline": res, "streaming": streaming(m, dec, mel, args, audio_s)}
        out["runs"].append(run)
        print(json.dumps(run), flush=True)
        del mel
        torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
