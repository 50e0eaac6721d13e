#!/usr/bin/env python3
"""Per-request hotwords (INTEGRATION.md "Per-request hotwords") at the decode shape of tools/ctc_beam_hotword_bench.py: B = 32,
T = 249, V = 370, 20 synthetic phrases of 1 to 3 words per list, hotword_weight = 9, W in {100, 190}, K = 16, random and peaky
logits, with and without the synthetic 5-gram.  Device time per call from HIP events:

  (a) shared     the existing search with one list for the launch (cfm_ctc_beam_hw_decode_f32)
  (b) rows_one   the per-row entry with all 32 rows pointing at ONE table (tables and arrays uploaded before the timing)
  (c) rows_32    the per-row entry with 32 different lists
  (c') rows_32_call   (c) through beam_ctc_hotword_decode(hotwords=[32 lists]): packing and the upload included (host + device)
  (d) slots      SlotTranscriber.open(s, hotwords=...) host time beside open(s) of an object without slot_hotwords, and the wall
                 time of the step that follows (32 slots, a tiny model: the search is the same, the encoder is not the subject)

Each figure is the median of --rounds rounds of --iters calls after a warm-up, with the rounds' minimum and maximum; the variants
of one case are timed in turn within every round, so drift hits them alike.  --parent-lib PATH times (a) again through the same
entry of ANOTHER build of the library (the parent commit's), interleaved with this one's in every round: `shared_parent`,
beside `shared_raw`, this build's entry called the same way (a bare ctypes call with its own output buffers), so that the pair
differs in the library alone.

    python tools/hotword_rows_bench.py [--iters 20] [--rounds 7] [--no-lm] [--parent-lib PATH] [--out profiles/hotword_rows_bench.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conformer_amd import _lib, ops  # noqa: E402
from conformer_amd.decode import BeamCTCDecoder, _Fusion, _beam_search, beam_ctc_hotword_decode  # noqa: E402
from conformer_amd.hotwords import HotwordRows, Hotwords  # noqa: E402
from conformer_amd.lm import NgramLanguageModel, write_synthetic_arpa  # noqa: E402
from tools.ctc_beam_hotword_bench import B, COUNTS, N_PHRASES, T, WIDTHS, graphemes, logits_for  # noqa: E402

KNOBS = dict(token_min_logp=-5.0, beam_prune_logp=-10.0, max_candidates=16)
LMKNOBS = dict(alpha=2.1, beta=9.2, unk_score_offset=-10.0, score_boundary=True)
WEIGHT = 9.0


def events(fn, iters: int) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def interleaved(variants: dict, iters: int, rounds: int) -> dict:
    """name -> {median, min, max} ms per call; every round times every variant once, in the given order"""
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    seen = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            seen[k].append(events(fn, iters))
    return {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in seen.items()}


def raw_entry(path: str):
    """cfm_ctc_beam_hw_decode_f32 of a build of the library (this one's or another), bound from this tree's header"""
    lib = ctypes.CDLL(path)
    fn = lib.cfm_ctc_beam_hw_decode_f32
    fn.restype, fn.argtypes = _lib.ENTRIES["cfm_ctc_beam_hw_decode_f32"]
    return fn


def search_case(x, L, W, vocab, lm, shared: Hotwords, lists, parent, iters, rounds):
    dev = x.device
    skip = (2,)
    lm_tables = None if lm is None else lm.device_tables(vocab, "|", skip, dev)

    def fusion(rows=None, hw=None):
        return lambda _dev: _Fusion(lm_tables, hw, **LMKNOBS, hotword_weight=WEIGHT, rows=rows)

    def search(f):
        return lambda: _beam_search(x, 0, L, 1, W, KNOBS["token_min_logp"], KNOBS["beam_prune_logp"], KNOBS["max_candidates"],
                                    vocab, f)

    one = HotwordRows([shared] * B, WEIGHT, vocab, "|", skip).to_device(dev)
    many = HotwordRows(lists, WEIGHT, vocab, "|", skip)
    many_dev = many.to_device(dev)
    variants = {"shared": search(fusion(hw=shared.device_tables(vocab, "|", skip, dev)))}
    if parent is not None:
        ws_bytes = int(_lib.load().cfm_ctc_beam_workspace_bytes(B, T, W, KNOBS["max_candidates"]))
        f = fusion(hw=shared.device_tables(vocab, "|", skip, dev))(dev)

        def raw(entry):
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            tokens = torch.empty(B, 1, T, dtype=torch.int64, device=dev)
            counts = torch.empty(B, 1, dtype=torch.int64, device=dev)
            scores, am = (torch.empty(B, 1, dtype=torch.float32, device=dev) for _ in range(2))
            num = torch.empty(B, dtype=torch.int64, device=dev)
            st = entry(x.data_ptr(), L.data_ptr(), B, T, x.shape[2], 0, W, KNOBS["max_candidates"], KNOBS["token_min_logp"],
                        KNOBS["beam_prune_logp"], 1, *f.args, ws.data_ptr(), ws_bytes, tokens.data_ptr(), counts.data_ptr(),
                        scores.data_ptr(), am.data_ptr(), num.data_ptr(), ops._stream())
            if st:
                raise RuntimeError(f"cfm_ctc_beam_hw_decode_f32 through ctypes returned {st}")
            return tokens, counts, scores, am, num
        this = raw_entry(_lib.LIB_PATH)
        variants["shared_raw"] = lambda: raw(this)
        variants["shared_parent"] = lambda: raw(parent)
        a, b = variants["shared"](), variants["shared_parent"]()
        assert all(torch.equal(u, v) for u, v in zip(a, b)), "this build and the parent's disagree on the shared-list search"
    variants["rows_one"] = search(fusion(rows=one))
    variants["rows_32"] = search(fusion(rows=many_dev))
    variants["rows_32_call"] = lambda: beam_ctc_hotword_decode(x, 0, lists, L, vocab=vocab, skip_ids=skip, hotword_weight=WEIGHT,
                                                               lm=lm, beam_width=W, **KNOBS, **LMKNOBS)
    a, b = variants["shared"](), variants["rows_one"]()
    assert all(torch.equal(u, v) for u, v in zip(a, b)), "32 rows on one table must equal the shared-list search"
    r = interleaved(variants, iters, rounds)
    r["distinct_tables"], r["table_bytes"] = many.distinct, int(many.blob.nbytes)
    return r


def slots_case(vocab, lists, dev, rounds):
    """(d): the host time of open(s, hotwords=...) and the wall time of the step after it, beside an object without lists"""
    from conformer_amd.slots import SlotTranscriber
    from model.conformer import Conformer
    torch.manual_seed(0)
    m = Conformer(len(vocab), 80, 2, 32, 4, 31, 24, 1, 0.0).to(dev).eval()
    dec = BeamCTCDecoder(vocab, 0, skip_ids=(2,), beam_width=100, beam_prune_logp=-10.0)
    P, C = max(len(Hotwords(h)) for h in lists), max(Hotwords(h).code_points for h in lists)
    out = {"slots": B, "reserved": [P, C]}
    mel = torch.randn(B, 80, 64, generator=torch.Generator().manual_seed(1)).mul(3.0).to(dev)
    for name, kw in (("with_lists", dict(slot_hotwords=(P, C))), ("without", {})):
        tr = SlotTranscriber(m, dec, B, 4000, **kw)
        opens, steps = [], []
        for r in range(rounds + 1):
            torch.cuda.synchronize()
            for s in range(B):
                t0 = time.perf_counter()
                tr.open(s, lists[s], WEIGHT) if kw else tr.open(s)
                opens.append(time.perf_counter() - t0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.step(mel, [64] * B)
            torch.cuda.synchronize()
            steps.append(time.perf_counter() - t0)
            for s in range(B):
                tr.close(s)
        opens, steps = opens[B:], steps[1:]                                   # (the first round warms up)
        out[name] = {"open_host_us": {"median": round(1e6 * statistics.median(opens), 1), "max": round(1e6 * max(opens), 1)},
                     "step_wall_ms": {"median": round(1e3 * statistics.median(steps), 3), "min": round(1e3 * min(steps), 3),
                                      "max": round(1e3 * max(steps), 3)}}
        if kw:
            out["region_bytes"] = tr.beam.state.regions.stride
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-lm", action="store_true", help="skip the runs fused with the 5-gram")
    ap.add_argument("--parent-lib", default=None, help="another build of libconformer_hip.so to time (a) through as well")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hotword_rows_bench: no HIP device (the decode only runs on the GPU; there is nothing to time here)")
    dev = torch.device("cuda:0")
    toks = graphemes(367)
    vocab = ["<pad>", "|", "<unk>"] + toks
    t0 = time.time()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "synthetic5.arpa")
        words = write_synthetic_arpa(path, toks, 20_000, COUNTS if not args.no_lm else [0, 10], seed=0)
        lm = None if args.no_lm else NgramLanguageModel.from_arpa(path)
    rng = np.random.default_rng(1)

    def phrases():
        return [" ".join(rng.choice(words, size=int(rng.integers(1, 4)))) for _ in range(N_PHRASES)]
    shared = Hotwords(phrases())                                              # the list of tools/ctc_beam_hotword_bench.py
    lists = [phrases() for _ in range(B)]
    parent = None if args.parent_lib is None else raw_entry(args.parent_lib)
    L = torch.full((B,), T, dtype=torch.int64, device=dev)
    out = {"B": B, "T": T, "V": len(vocab), "K": 16, "iters": args.iters, "rounds": args.rounds, "phrases": N_PHRASES,
           "hotword_weight": WEIGHT, "lm_ngrams": None if lm is None else sum(lm.counts), "device": torch.cuda.get_device_name(0),
           "parent_lib": args.parent_lib is not None, "setup_s": round(time.time() - t0, 1), "ms": {}}
    for kind in ("random", "peaky"):
        x = logits_for(kind, len(vocab), dev)
        out["ms"][kind] = {}
        for W in WIDTHS:
            r = {"lm_free": search_case(x, L, W, vocab, None, shared, lists, parent, args.iters, args.rounds)}
            if lm is not None:
                r["lm"] = search_case(x, L, W, vocab, lm, shared, lists, parent, args.iters, args.rounds)
            out["ms"][kind][str(W)] = r
            print(f"[hotword_rows_bench] {kind} W={W}: {json.dumps(r)}", file=sys.stderr, flush=True)
    out["slots"] = slots_case(vocab, lists, dev, args.rounds)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
