"""Chunk-by-chunk (streaming) evaluation of the Encoder with cached K/V and depthwise-convolution state -- BASELINE cfg-5
("T=20000 in 640-frame chunks with cached K/V + depthwise state").

The reference has no streaming code at all, so there is nothing to be identical to chunk by chunk; the semantics chosen are
the ones its own operators already have at the END of an utterance, applied at the end of every chunk (the prefix rule):

    an encoder frame that belongs to chunk c is computed, in every layer, from the frames of chunks <= c only --
    self-attention sees the keys received so far (the same key limit `lengths` gives Encoder.forward), the depthwise
    convolution treats the not-yet-received frames as the zero padding of convolution.py:14.

Consequences that the tests pin: one chunk holding the whole utterance IS Encoder.forward; the frames of the first chunk
equal Encoder.forward of that prefix alone; any chunking equals the masked whole-sequence restatement
`oracle.encoder_forward_chunked` (float64).  The conv-subsampling stem, the input Linear, LayerNorm and the feed-forward
modules are local in time, so they are exact under chunking; relative positions need no absolute frame index.

State per layer: the fused Q|K|V projections of every frame so far (B, T'max, 3d) -- new rows are appended in place and
`cfm_relpos_attention_rows_f32` computes the new query rows only, against the whole cache -- and the last (K-1)/2 GLU
outputs feeding the depthwise convolution.  Per utterance: the un-consumed tail (3..6 frames) of the mel stream and the
positional table projected ONCE for T'max.

Bounded history (`left_context=L`, INTEGRATION.md "Bounded history"): the windowed prefix rule -- query frame i of a chunk that
ends at frame e attends to the keys max(0, i-L) <= j < e; everything else above stays.  The per-layer caches are then RINGS
(B, R, 3d), frame n in row n mod R, R = 32 ceil((L + k_cap)/32) with k_cap the most encoder frames one step can make; the table is
projected for P = max(L+1, k_cap) positions and `cfm_relpos_attention_window_f32` attends.  Memory and the cost of a chunk no
longer depend on the stream position, and max_mel_frames may be None: a stream without an end.
"""
from __future__ import annotations

from typing import Iterable, List, Optional

import torch

from . import ops
from ._derived import fingerprint
from .model.modules.encoder import Encoder


def ring_plan(left_context: int, max_chunk_mel_frames: int):
    """(R, P, k_cap) of a windowed stream: a step buffers at most 6 + max_chunk_mel_frames mel frames, so it makes at most k_cap
    encoder frames; the ring keeps the L frames a query may look back on next to the step's own rows, in whole key tiles of 32;
    the table covers the relative positions -(k_cap-1) .. L.  Host arithmetic."""
    L, mc = int(left_context), int(max_chunk_mel_frames)
    if L < 0:
        raise ValueError(f"left_context must be >= 0 encoder frames, got {L}")
    if mc < 1:
        raise ValueError(f"max_chunk_mel_frames must be >= 1, got {mc}")
    k_cap = encoder_frames(mc + 6)
    return 32 * ((L + k_cap + 31) // 32), max(L + 1, k_cap), k_cap


def ring_rows(n0: int, k: int, R: int):
    """Ring rows of frames n0 .. n0+k-1 (k <= R) as one or two (ring start, source start, count) runs."""
    s = n0 % R
    first = min(k, R - s)
    return [(s, 0, first)] + ([(0, first, k - first)] if first < k else [])


def _window_args(who: str, left_context, max_chunk_mel_frames, max_mel_frames):
    """The three sizing keywords of the streaming objects, checked on the host: (L, max chunk) or (None, None)."""
    if left_context is None:
        if max_chunk_mel_frames is not None:
            raise ValueError(f"{who}: max_chunk_mel_frames sizes the ring of a windowed stream: give left_context too")
        if max_mel_frames is None:
            raise ValueError(f"{who}: max_mel_frames=None (a stream without an end) needs left_context")
        return None, None
    if max_chunk_mel_frames is None:
        raise ValueError(f"{who}: left_context needs max_chunk_mel_frames (the ring is sized for the largest step)")
    ring_plan(left_context, max_chunk_mel_frames)
    return int(left_context), int(max_chunk_mel_frames)


def _refuse_window_autocast(who: str) -> None:
    if torch.is_autocast_enabled("cuda"):
        raise NotImplementedError(f"{who}: left_context is fp32 only (no 16-bit window kernel yet); leave torch.autocast")


def encoder_frames(mel_frames: int) -> int:
    """Encoder frames the stem makes of `mel_frames` mel frames (convolution.py:55; <= 0: none yet).  Host arithmetic, per step."""
    return ((mel_frames - 1) // 2 - 1) // 2


class _Stream:
    """The stream context of ConformerBlock.fused_chain for one lockstep chunk step: the chunk is rows n0 .. n0+k-1 of every
    utterance; `i` is the layer the chain is in (ChunkedEncoder._encode sets it)."""

    qkv16 = False              # the K/V cache is fp32: the q|k|v GEMM writes fp32 rows (slots.py: a 16-bit cache sets it)

    def __init__(self, st: "StreamingEncoder", n0: int, k: int) -> None:
        self.st, self.n0, self.k, self.i = st, n0, k, 0
        self._pos = None           # windowed: (q_begin, q_count) on the device, made once per step

    def attend(self, a, qkv_new: torch.Tensor) -> torch.Tensor:
        """Append the chunk's Q|K|V rows to the layer's cache and return the attention context of the new rows (B, k, d)."""
        st, i, n0, k = self.st, self.i, self.n0, self.k
        if st.left is not None:                                            # ring: rows (n0 + r) mod R, then the window kernel
            for dst, src, n in ring_rows(n0, k, st.ring):
                st.qkv[i][:, dst:dst + n].copy_(qkv_new[:, src:src + n])
            if self._pos is None:
                dev = qkv_new.device
                self._pos = (torch.full((st.B,), n0, dtype=torch.int64, device=dev),
                             torch.full((st.B,), k, dtype=torch.int64, device=dev))
            return ops.relpos_attention_window(st.qkv[i], st.pos_all[:, i * st.d:(i + 1) * st.d], a.content_bias, a.position_bias,
                                               a.n_heads, self._pos[0], self._pos[1], k, st.left)
        st.qkv[i][:, n0:n0 + k].copy_(qkv_new)
        ops.relpos_attention_rows(st.qkv[i], st.pos_all[:, i * st.d:(i + 1) * st.d], a.content_bias, a.position_bias,
                                  st.lengths, a.n_heads, n0, k, st.ctx, keys_hint=n0 + k)
        return st.ctx[:, n0:n0 + k].contiguous()

    def depthwise(self, cv, g: torch.Tensor) -> torch.Tensor:
        """The depthwise window reaches (K-1)/2 frames back into the layer's carried GLU rows; the last (K-1)/2 rows are
        carried into the next chunk (a fixed buffer: the graph replays write the same address)."""
        state = self.st.conv_state[self.i]
        half = state.shape[1]
        buf = torch.cat([state, g], dim=1)                                 # (B, half + k, C)
        s = cv.depthwise_eval(buf)
        state.copy_(buf[:, buf.shape[1] - half:])
        return s[:, half:].contiguous()


class ChunkedEncoder:
    """What StreamingEncoder and slots.SlotStreamingEncoder share (`who`: the one the messages name): the checks, the ring
    sizing, the K/V caches (linear (B, T'max, 3d) or rings (B, R, 3d), stored as `cache_dtype`), depthwise state, key limits,
    mel tail buffer, what is derived from the weights and the chain over the blocks.  How a step places its rows is theirs."""

    def __init__(self, who: str, encoder: Encoder, batch: int, max_mel_frames: Optional[int], check_weights: bool = True,
                 cache_dtype: torch.dtype = torch.float32, *, left_context: Optional[int] = None,
                 max_chunk_mel_frames: Optional[int] = None) -> None:
        self.left, self.max_chunk = _window_args(who, left_context, max_chunk_mel_frames, max_mel_frames)
        if encoder.training:
            raise RuntimeError(f"{who}: put the encoder in eval() mode (running BatchNorm statistics, no dropout)")
        p = next(encoder.parameters())
        if not p.is_cuda or p.dtype != torch.float32:
            raise RuntimeError(f"{who}: the encoder must live on the HIP device in fp32 (no CPU fallback)")
        self.enc = encoder
        self.B = int(batch)
        self.d = encoder.linear.out_features
        self.t_max = None if max_mel_frames is None else encoder_frames(int(max_mel_frames))     # None: a stream without an end
        if self.t_max is not None and self.t_max < 1:
            raise ValueError("max_mel_frames must give at least one encoder frame (>= 7)")
        dev = p.device
        layers = list(encoder.layers)
        self.ring, self.n_pos, _ = (None, None, None) if self.left is None else ring_plan(self.left, self.max_chunk)
        self.qkv = [torch.zeros(self.B, self.ring or self.t_max, 3 * self.d, device=dev, dtype=cache_dtype) for _ in layers]
        halves = [(l.conv.deepwise_conv.kernel_size[0] - 1) // 2 for l in layers]     # the carried GLU rows: (K-1)/2 per layer
        self.conv_state = [torch.zeros(self.B, h, self.d, device=dev, dtype=torch.float32) for h in halves]
        self.lengths = torch.zeros(self.B, dtype=torch.int64, device=dev)
        self.mel_tail_buf: Optional[torch.Tensor] = None                   # (B, n_mel, 8): the un-consumed 0..6 mel frames
        self.check_weights = bool(check_weights)
        self._tensors = list(encoder.parameters()) + list(encoder.buffers())     # (walked once, not per step)
        self._derive()

    @torch.no_grad()
    def _derive(self) -> None:
        """Everything this object holds that was made from the weights (a subclass that holds more extends this)."""
        self.table = self.enc.rel_pe.table(self.t_max if self.left is None else self.n_pos)
        self.pos_all = self.enc._projected_positions(self.table)          # (2T'max-1 | 2P-1, L*d): every layer's pos_proj, once
        self._fingerprint = fingerprint(self._tensors)

    def _follow_weights(self) -> None:
        """The top of every step: weights changed since _derive() -- never run on a stale table or replay stale packs."""
        if self.check_weights and fingerprint(self._tensors) != self._fingerprint:
            self._derive()

    def _encode(self, mel: torch.Tensor, stream, set_lengths) -> torch.Tensor:
        """Stem, input Linear and the blocks on the mel frames of a step's new encoder frames (the stem is local in time);
        `stream` takes the new rows through the two seams of every block (ConformerBlock.fused_chain); set_lengths() enqueues
        the step's key limits (self.lengths) in front of the blocks."""
        enc = self.enc
        h = enc.downsampling_conv.channel_last(mel.contiguous())           # (B, k, F'*C)
        wlp = enc._packs.get("wlp", (enc.linear.weight,), lambda: ops.pack_linear_weight(enc.linear.weight, self.d, enc.n_freq_out))
        h = ops.linear(h, wlp, enc.linear.bias)
        set_lengths()
        stats = None
        for i, blk in enumerate(enc.layers):
            stream.i = i
            h, stats = blk.fused_chain(h, None, None, x_stats=stats, want_stats=i + 1 < len(enc.layers), stream=stream)
        return h


class StreamingEncoder(ChunkedEncoder):
    """graphs=True: every distinct chunk step -- keyed on (frames so far, chunk length, buffered tail, matrix-pipe precision) -- is
    captured ONCE as a hipGraph and replayed from then on (the next utterance batch of a streaming service walks through the same
    keys): one host call per chunk instead of ~420 launches, whose issue cost (not their device time) was what a 7-11 ms chunk
    step consisted of (profiles/r02_streaming_bench.json vs r03).  All graphs share one memory pool; the state (K/V caches,
    depthwise state, mel tail) lives in fixed buffers outside it.  The returned frames are a copy (the graph's output buffer is
    reused).

    The projected position table and the graphs hold what was derived from the weights when they were made.  Every step()
    compares the encoder's fingerprint (epoch, address and in-place version of each parameter and buffer, as GraphedEncoder
    does) with the recorded one; after an optimizer step, `load_state_dict`, an in-place update or invalidate_weight_caches()
    the table is projected again and all graphs are dropped, eager path included.  The stream state is NOT touched: the cached
    K/V rows were computed with the old weights, so a caller who changes weights mid-utterance calls reset().
    check_weights=False (frozen-weight serving) skips that per-step walk over the encoder's tensors.

    left_context=L (encoder frames, with max_chunk_mel_frames: the most mel frames one step() may bring): bounded history, the
    module docstring's windowed rule over ring caches; max_mel_frames may then be None (no end).  fp32 and eager only: graphs=True
    or a step under torch.autocast raises NotImplementedError."""

    def __init__(self, encoder: Encoder, batch: int, max_mel_frames: Optional[int] = None, graphs: bool = False,
                 check_weights: bool = True, *, left_context: Optional[int] = None,
                 max_chunk_mel_frames: Optional[int] = None) -> None:
        if left_context is not None and graphs:
            raise NotImplementedError("StreamingEncoder: graphs=True with left_context (a graph key still holds the stream "
                                      "position, so an endless stream would capture without end)")
        super().__init__("StreamingEncoder", encoder, batch, max_mel_frames, check_weights, left_context=left_context,
                         max_chunk_mel_frames=max_chunk_mel_frames)
        self.ctx = None                    # the rows kernel's scratch, shared by the layers (windowed: compact, per step)
        if self.left is None:
            self.ctx = torch.zeros(self.B, self.t_max, self.d, device=self.lengths.device, dtype=torch.float32)
        self.tail_len = 0
        self.frames = 0                                                    # encoder frames produced so far
        self.use_graphs = bool(graphs)

    def _derive(self) -> None:                                             # and the graphs and their pool: they replay the weights
        super()._derive()
        self._graphs = {}                                                  # key -> (graph, static input, static output)
        self._pool = None
        self._warm = set()                                                 # precisions whose derived weights a warm step built

    def reset(self) -> None:
        for t in self.conv_state:
            t.zero_()
        self.tail_len = 0
        self.frames = 0

    @property
    def mel_tail(self) -> Optional[torch.Tensor]:
        return None if self.tail_len == 0 or self.mel_tail_buf is None else self.mel_tail_buf[:, :, :self.tail_len]

    @torch.no_grad()
    def step(self, mel_chunk: torch.Tensor) -> torch.Tensor:
        """mel_chunk (B, n_mel, Tc): the next Tc log-mel frames of every utterance (any Tc >= 1).  Returns the encoder
        frames that became computable, (B, k, d) with k = ((buffered-1)//2-1)//2 >= 0."""
        if self.left is not None:                                          # refusals first: nothing enqueued, no state touched
            _refuse_window_autocast("StreamingEncoder")
            if mel_chunk.shape[2] > self.max_chunk:
                raise ValueError(f"StreamingEncoder: a step of {mel_chunk.shape[2]} mel frames, the ring was sized for "
                                 f"max_chunk_mel_frames={self.max_chunk}")
        self._follow_weights()
        x_in = ops._req(mel_chunk, "mel_chunk")
        if self.mel_tail_buf is None:
            self.mel_tail_buf = torch.zeros(self.B, x_in.shape[1], 8, device=x_in.device, dtype=torch.float32)
        n0, tail = self.frames, self.tail_len
        total = tail + x_in.shape[2]
        k = max(0, encoder_frames(total))
        if k <= 0:
            # not enough frames for one encoder frame yet: just buffer (<= 6 frames; tiny copy, never graphed)
            self.mel_tail_buf[:, :, tail:total].copy_(x_in)
            self.tail_len = total
            return x_in.new_empty(self.B, 0, self.d)
        if self.t_max is not None and n0 + k > self.t_max:
            raise RuntimeError(f"StreamingEncoder: stream longer than max_mel_frames (T'max = {self.t_max})")
        if not self.use_graphs:
            out = self._step_core(x_in, n0, tail, k)
        else:
            prec = ops.mfma16_prec()                                      # the capture bakes in the fp32 or the 16-bit kernels
            key = (n0, x_in.shape[2], tail, prec)
            ent = self._graphs.get(key)
            if ent is None:
                if self._pool is None:
                    self._pool = torch.cuda.graph_pool_handle()
                if prec not in self._warm:
                    self._warm.add(prec)
                    self._step_warm(x_in, n0, tail, k)                    # derived weights / tables are built outside any capture
                static_in = x_in.clone()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, pool=self._pool):
                    static_out = self._step_core(static_in, n0, tail, k)
                ent = self._graphs[key] = (g, static_in, static_out)
            else:
                ent[1].copy_(x_in)
            ent[0].replay()
            out = ent[2].clone()
        self.tail_len = total - 4 * k
        self.frames = n0 + k
        return out

    def _step_warm(self, x_in: torch.Tensor, n0: int, tail: int, k: int) -> None:
        """One eager step whose effects on the state are undone (it overwrites cache rows the real step rewrites; the mel tail and
        the depthwise state are restored)."""
        keep_tail = self.mel_tail_buf.clone()
        keep_conv = [t.clone() for t in self.conv_state]
        self._step_core(x_in, n0, tail, k)
        self.mel_tail_buf.copy_(keep_tail)
        for t, kt in zip(self.conv_state, keep_conv):
            t.copy_(kt)
        torch.cuda.synchronize()

    def _step_core(self, x_in: torch.Tensor, n0: int, tail: int, k: int) -> torch.Tensor:
        """The device work of one chunk: capture-safe (fixed state buffers, no host synchronisation, no data-dependent shapes)."""
        x = x_in if tail == 0 else torch.cat([self.mel_tail_buf[:, :, :tail], x_in], dim=2)
        # encoder frame t covers mel frames 4t .. 4t+6: the buffer starts at mel frame 4*n0, keep what frame n0+k needs
        rest = x.shape[2] - 4 * k
        self.mel_tail_buf[:, :, :rest].copy_(x[:, :, 4 * k:])
        return self._encode(x, _Stream(self, n0, k), lambda: self.lengths.fill_(n0 + k))

    def run(self, mel: torch.Tensor, chunk_frames: int = 640) -> torch.Tensor:
        """Feeds mel (B, n_mel, T) in chunks of `chunk_frames` and returns the concatenated (B, T', d) output."""
        outs: List[torch.Tensor] = [self.step(mel[:, :, t:t + chunk_frames]) for t in range(0, mel.shape[2], chunk_frames)]
        return torch.cat(outs, dim=1)


def chunk_ends(total_mel_frames: int, chunk_frames: Iterable[int]) -> List[int]:
    """Encoder-frame boundaries produced by feeding chunks of the given sizes (for comparing with the masked restatement)."""
    ends, got = [], 0
    for c in chunk_frames:
        got += c
        n = encoder_frames(got)
        if n > 0 and (not ends or n > ends[-1]):
            ends.append(n)
    return ends
