#!/usr/bin/env python3
"""Long-form CTC forced alignment (conformer_amd.align.ctc_forced_align_long): the chain launches and the whole call.

    (T, L) = (16384, 4096)   the largest shape ctc_forced_align takes, beside ctc_forced_align on the same logits and targets
    (90000, 30000)           one hour of audio with a dense transcript: over a grid of tile_pairs x chunk_frames
    (90000, 10000)           one hour with a sparse one: many cells can no longer reach the end (back-dead)

B = 1, V = 370 (the reference vocabulary).  Device time per call from HIP events after a warm-up; `chain_ms` is the chain
stage alone (feasibility, the n_tiles + n_chunks - 1 cell launches, the end state: cfm2_ctc_align_long_chain_f32 into the same
workspace), `align_ms` the whole call including the workspace allocation.  `dead_cells` is the share of the launched cells that
are skipped whole (front- plus back-dead, counted on the host with the kernel's rule).  The fastest pair at (90000, 30000) is
what the library's defaults are set to.  Writes profiles/ctc_align_long_bench.json and prints it as one JSON line.

    python tools/ctc_align_long_bench.py [--iters 5] [--quick]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from conformer_amd import _lib, ops  # noqa: E402
from conformer_amd.align import ctc_forced_align, ctc_forced_align_long, long_workspace_bytes  # noqa: E402

V = 370
GRID = [(512, 128), (512, 256), (512, 512), (1024, 256), (1024, 512), (2048, 256), (2048, 512), (2048, 1024), (4096, 512),
        (8192, 1024)]


def time_ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / iters, 3)


def dead_cells(T, L, tp, cf):
    """(cells, front-dead, back-dead) of one utterance with T frames and L labels, by align_long_cell_kernel's rule"""
    cells = front = back = 0
    for k in range(-(-(L + 1) // tp)):
        for c in range(-(-T // cf)):
            t_first, t_end, i_first = c * cf, min(c * cf + cf, T), k * tp
            cells += 1
            if i_first > t_end - 1:
                front += 1
            elif L - 1 - (i_first + tp - 1) > T - 1 - t_first:
                back += 1
    return cells, front, back


def measure(x, y, T, L, tp, cf, iters):
    lib = _lib.load()
    ws_bytes = long_workspace_bytes(1, T, L, tp, cf)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)

    def chain():
        _lib.call("cfm2_ctc_align_long_chain_f32", x.data_ptr(), y.data_ptr(), None, None, 1, T, V, L, 0, tp or 0, cf or 0,
                  ws.data_ptr(), ws_bytes, ops._stream())

    cells, front, back = dead_cells(T, L, tp, cf) if tp else (0, 0, 0)
    res = {"tile_pairs": tp, "chunk_frames": cf, "launches": int(lib.cfm2_ctc_align_long_launches(T, L, tp or 0, cf or 0)),
           "workspace_mb": round(ws_bytes / 2 ** 20, 1),
           "chain_ms": time_ms(chain, iters)}
    del ws
    res["align_ms"] = time_ms(lambda: ctc_forced_align_long(x, y, 0, tile_pairs=tp, chunk_frames=cf), iters)
    if cells:
        res["dead_cells"] = round((front + back) / cells, 3)
        res["front_dead"], res["back_dead"] = front, back
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="three tilings per one-hour shape instead of the grid")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ctc_align_long_bench: no HIP device (the alignment only runs on the GPU; there is nothing to time here)")
    dev = torch.device("cuda:0")
    grid = GRID[1::4] if args.quick else GRID
    out = {"iters": args.iters, "V": V, "shapes": {}}
    for name, T, L in (("old_limit", 16384, 4096), ("hour_dense", 90000, 30000), ("hour_sparse", 90000, 10000)):
        g = torch.Generator().manual_seed(0)
        x = (torch.randn(1, T, V, generator=g) * 2).to(dev)
        y = torch.randint(1, V, (1, L), generator=g).to(dev)
        assert bool(ctc_forced_align_long(x, y, 0).ok.all())
        res = {"T": T, "L": L, "tilings": [measure(x, y, T, L, tp, cf, args.iters) for tp, cf in grid]}
        res["fastest"] = min(res["tilings"], key=lambda r: r["chain_ms"])
        res["defaults"] = measure(x, y, T, L, None, None, args.iters)
        if name == "old_limit":
            res["ctc_forced_align_ms"] = time_ms(lambda: ctc_forced_align(x, y, 0), args.iters)
            res["long_over_short"] = round(res["defaults"]["align_ms"] / res["ctc_forced_align_ms"], 3)
        out["shapes"][name] = res
        del x, y
        torch.cuda.empty_cache()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "ctc_align_long_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
