"""Offline transcription of recordings of any length: overlapped windows through the full-context encoder (INTEGRATION.md
"Offline and long-form transcription").

Encoder.forward attends over its whole input, so a one-hour recording would be one attention over ~90 000 frames.  Here a
recording is cut into fixed windows of W mel frames that overlap by O; the windows of all recordings run through the encoder as
ordinary (B, n_mel, W) batches -- the shape it is fastest at -- and every encoder frame of the recording is taken from the window
in which it has the most context on both sides.  The decoder head, the beam search and the confidences then run once over the
stitched frames of the whole recording, so word times are global by construction.

Three layers: window_plan (host arithmetic), BufferedEncoder (mel frames in, stitched encoder frames out) and Transcriber
(waveforms or mel frames in, Transcripts out).  Transcriber.align puts a KNOWN transcript on the time axis of a whole recording
(align.ctc_forced_align_long on the stitched frames) and cut_utterances cuts the aligned words into training utterances;
Transcriber.segments locates given utterances in a recording that holds other audio too (wildcards between them).
Transcriber(vad=VadConfig(...)) puts the voice activity detector (conformer_amd.vad) in front of the plan: only the speech
islands of a recording are encoded, and the words keep the recording's own times.
There is no kernel of its own in here: the hot path is Encoder.forward, the decoder head, the search and the aligner, which
are gfx950 kernels already; the plan, the batching and the stitching are slices and copies.
"""
from __future__ import annotations

import math
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from .align import CTCAligner, Segment, Word
from .confidence import ConfidenceConfig, frame_confidence, transcriber_confidence, word_confidence
from .decode import BeamCTCDecoder
from .frontend import ConformerAudioFrontend
from .graph import GraphedEncoder
from .streaming import encoder_frames
from .transcribe import lstm_state, times_plan

MIN_MEL_FRAMES = 7                      # the fewest mel frames the stem makes an encoder frame of


class Window(NamedTuple):
    """One window of a plan.  It reads the mel frames [start, start + mel) and makes the encoder frames [first, first +
    encoder_frames(mel)) of the recording's own grid (first = start / 4); the rows [keep_from, keep_to) of that grid are taken
    from it, which are its local rows [keep_from - first, keep_to - first)."""
    start: int
    mel: int
    first: int
    keep_from: int
    keep_to: int


def check_window(window: int, overlap: int) -> Tuple[int, int]:
    """Refuse a window / overlap pair (mel frames) that window_plan cannot tile with; returns (W, H), H = W - O the hop."""
    for name, v in (("window", window), ("overlap", overlap)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"window_plan: {name} must be a number of mel frames, got {v!r}")
    W, H = window, window - overlap
    if W < 12:
        raise ValueError(f"window_plan: window = {W} mel frames, the least is 12 (a right-aligned last window may be 3 shorter and "
                         f"still has to make an encoder frame)")
    if H < 4:
        raise ValueError(f"window_plan: window - overlap = {H} mel frames, the least is 4 (one encoder frame)")
    if H % 4:
        raise ValueError(f"window_plan: window - overlap = {H} mel frames is no multiple of 4 (window starts have to fall on the "
                         "encoder's frame grid)")
    if encoder_frames(W) < H // 4:
        raise ValueError(f"window_plan: a window of {W} mel frames makes {encoder_frames(W)} encoder frames, consecutive windows "
                         f"start {H // 4} apart: they would leave a gap (raise overlap)")
    return W, H


def window_plan(n_mel: int, window: int, overlap: int) -> List[Window]:
    """The windows of a recording of n_mel mel frames, `window` = W and `overlap` = O in mel frames, H = W - O.

    One window (0, n_mel) if n_mel <= W.  Otherwise ceil((n_mel - W) / H) + 1 windows: window i starts at i * H and is W long,
    except the last, which is right-aligned: it starts at 4 * ceil((n_mel - W) / 4) and runs to the end (W - 3 .. W frames).
    Every start is a multiple of 4, so the local encoder frame j of a window that starts at s is the frame s / 4 + j of the
    recording's own grid (frame j covers the mel frames s + 4j .. s + 4j + 6) and the last window ends at encoder_frames(n_mel).
    Consecutive windows are cut in the middle of the frames they share: window i keeps [c_(i-1), c_i) with
    c_i = first_(i+1) + (end_i - first_(i+1)) // 2; the first keeps from 0, the last up to encoder_frames(n_mel).  The kept
    ranges tile [0, encoder_frames(n_mel)) exactly once.

    ValueError for W < 12, H < 4, H % 4 != 0, encoder_frames(W) < H / 4 (a gap between windows) and n_mel < 7 (no encoder
    frame at all)."""
    W, H = check_window(window, overlap)
    if isinstance(n_mel, bool) or not isinstance(n_mel, int) or n_mel < MIN_MEL_FRAMES:
        raise ValueError(f"window_plan: a recording of {n_mel!r} mel frames makes no encoder frame (the least is {MIN_MEL_FRAMES})")
    if n_mel <= W:
        spans = [(0, n_mel)]
    else:
        n = -(-(n_mel - W) // H) + 1
        last = 4 * (-(-(n_mel - W) // 4))
        spans = [(i * H, W) for i in range(n - 1)] + [(last, n_mel - last)]
    first = [s // 4 for s, _ in spans]
    end = [a + encoder_frames(m) for a, (_, m) in zip(first, spans)]
    cuts = [0] + [first[i + 1] + (end[i] - first[i + 1]) // 2 for i in range(len(spans) - 1)] + [encoder_frames(n_mel)]
    return [Window(s, m, first[i], cuts[i], cuts[i + 1]) for i, (s, m) in enumerate(spans)]


def window_frames(window_seconds: float, overlap_seconds: float, mel_seconds: float) -> Tuple[int, int]:
    """(window, overlap) in mel frames of mel_seconds each for window_plan: the window is the most whole frames inside
    window_seconds, the hop W - O is rounded DOWN to a multiple of 4 frames, so that the overlap used is at least
    overlap_seconds.  Refuses (ValueError) what is no positive finite time, an overlap that is not shorter than the window and
    whatever window_plan refuses."""
    for name, v in (("window_seconds", window_seconds), ("overlap_seconds", overlap_seconds), ("mel_seconds", mel_seconds)):
        least = 0.0 if name == "overlap_seconds" else math.ulp(0.0)          # the overlap may be 0, the other two not
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < least:
            raise ValueError(f"window_frames: {name} must be a positive finite number of seconds, got {v!r}")
    if overlap_seconds >= window_seconds:
        raise ValueError(f"window_frames: overlap_seconds = {overlap_seconds} is not shorter than window_seconds = {window_seconds}")
    W = int(math.floor(window_seconds / mel_seconds + 1e-6))
    least = int(math.ceil(overlap_seconds / mel_seconds - 1e-6))
    H = (W - least) // 4 * 4
    check_window(W, W - H)
    return W, W - H


def _recording_hotwords(n: int, hotwords, hotword_weight):
    """transcribe's per-recording hotwords as (entries, weights), n of each, or None when neither was given."""
    if hotwords is None and hotword_weight is None:
        return None
    entries = [None] * n if hotwords is None else list(hotwords)
    if isinstance(hotwords, str) or len(entries) != n:
        raise ValueError(f"Transcriber: hotwords must have one entry per recording ({n}), got {len(entries)}")
    weights = list(hotword_weight) if isinstance(hotword_weight, (list, tuple)) else [hotword_weight] * n
    if len(weights) != n:
        raise ValueError(f"Transcriber: hotword_weight must be one float or one per recording ({n}), got {len(weights)}")
    return entries, weights


def _ambient_autocast(who: str) -> Optional[torch.dtype]:
    if not torch.is_autocast_enabled("cuda"):
        return None
    dt = torch.get_autocast_dtype("cuda")
    if dt not in (torch.bfloat16, torch.float16):
        raise RuntimeError(f"{who}: torch.autocast of {dt} has no gfx950 path (none, bfloat16 or float16)")
    return dt


class BufferedEncoder:
    """The encoder over recordings of any length, window by window (the module docstring).

        be = BufferedEncoder(model.encoder, window=3000, overlap=800); hs = be.encode([mel_a, mel_b])

    encoder: an Encoder in eval() mode on the HIP device.  window, overlap: mel frames, as window_plan takes them.  The windows
    of ALL recordings of a call are pooled, sorted by length (longest first, stable) and cut into batches of at most
    batch_windows.  A batch whose windows all have one length runs as encoder(x, None); a ragged one is zero-padded to its
    longest window and runs as encoder(x, lengths): an offline batch as it always was, so a list of recordings that each fit
    one window IS the reference's sorted, padded batch.  Each window's kept rows are then copied to their place in the
    recording's output.
    graphs=True: the full batches of full windows (batch_windows, n_mel, window) replay one captured graph (GraphedEncoder, one
    per ambient autocast type); everything else runs eagerly.  Changed weights are seen by the existing derived-weight rule
    (GraphedEncoder's fingerprint, the pack caches), there is nothing to call here.
    Under torch.autocast (bfloat16 / float16) the encoder runs its 16-bit path; the output keeps the encoder's dtype.

    Memory: beyond the inputs and the outputs (encoder_frames(n_i) x d floats per recording) a call holds ONE batch of windows:
    its input (batch_windows x n_mel x window floats), the activations of one Encoder.forward on it and its output
    (batch_windows x encoder_frames(window) x d floats), whatever the recordings' lengths; with graphs=True the captured graph
    keeps such a batch for the object's lifetime."""

    def __init__(self, encoder, window: int, overlap: int, batch_windows: int = 32, graphs: bool = False) -> None:
        self.window, self.hop = check_window(window, overlap)
        self.overlap = self.window - self.hop
        if isinstance(batch_windows, bool) or not isinstance(batch_windows, int) or batch_windows < 1:
            raise ValueError(f"BufferedEncoder: batch_windows must be a number of windows >= 1, got {batch_windows!r}")
        if not isinstance(graphs, bool):
            raise ValueError(f"BufferedEncoder: graphs must be True or False, got {graphs!r}")
        self.batch_windows, self.graphs = batch_windows, graphs
        self.encoder = encoder
        self._refuse()
        self._graphed: Dict[Optional[torch.dtype], GraphedEncoder] = {}

    def _refuse(self) -> torch.device:
        enc = self.encoder
        if enc.training:
            raise RuntimeError("BufferedEncoder: put the encoder in eval() mode (running BatchNorm statistics, no dropout)")
        p = next(enc.parameters())
        if not p.is_cuda or p.dtype != torch.float32:
            raise RuntimeError("BufferedEncoder: the encoder must live on the HIP device in fp32 (no CPU fallback)")
        return p.device

    def plan(self, mel_frames: Sequence[int]) -> List[List[Window]]:
        """window_plan of every recording."""
        return [window_plan(int(n), self.window, self.overlap) for n in mel_frames]

    def batches(self, plans: Sequence[Sequence[Window]]) -> List[List[Tuple[int, int]]]:
        """The pool of (recording, window index) pairs, sorted by mel length (longest first, stable), in batches."""
        pool = [(r, i) for r, ws in enumerate(plans) for i in range(len(ws))]
        pool.sort(key=lambda ri: -plans[ri[0]][ri[1]].mel)
        return [pool[k:k + self.batch_windows] for k in range(0, len(pool), self.batch_windows)]

    def _forward(self, x: torch.Tensor, lengths: Optional[torch.Tensor], amp: Optional[torch.dtype]) -> torch.Tensor:
        if self.graphs and lengths is None and x.shape[0] == self.batch_windows and x.shape[2] == self.window:
            if amp not in self._graphed:
                self._graphed[amp] = GraphedEncoder(self.encoder, x, None, autocast_dtype=amp)
            return self._graphed[amp](x, None)[0]
        return self.encoder(x, lengths)[0]

    @torch.no_grad()
    def encode(self, mels: Sequence[torch.Tensor]) -> List[torch.Tensor]:
        """mels: per recording its log-mel frames (n_mel, n_i), n_i >= 7 (on the device, or on the host: windows are copied
        over batch by batch).  Returns per recording its encoder frames (encoder_frames(n_i), d) on the device."""
        device = self._refuse()
        amp = _ambient_autocast("BufferedEncoder")
        mels = list(mels)
        for r, m in enumerate(mels):
            if not isinstance(m, torch.Tensor) or m.dim() != 2 or m.dtype != torch.float32:
                raise ValueError(f"BufferedEncoder: recording {r}: expected fp32 log-mel frames (n_mel, n), got "
                                 f"{tuple(m.shape) if isinstance(m, torch.Tensor) else type(m).__name__}")
            if m.shape[0] != mels[0].shape[0]:
                raise ValueError(f"BufferedEncoder: recording {r} has {m.shape[0]} mel channels, recording 0 has {mels[0].shape[0]}")
        plans = self.plan([m.shape[1] for m in mels])
        outs: List[Optional[torch.Tensor]] = [None] * len(mels)
        for batch in self.batches(plans):
            ws = [plans[r][i] for r, i in batch]
            longest = ws[0].mel
            ragged = ws[-1].mel != longest
            x = (torch.zeros if ragged else torch.empty)(len(ws), mels[0].shape[0], longest, device=device, dtype=torch.float32)
            for k, ((r, _), w) in enumerate(zip(batch, ws)):
                x[k, :, :w.mel].copy_(mels[r][:, w.start:w.start + w.mel], non_blocking=True)
            lengths = torch.tensor([w.mel for w in ws], dtype=torch.int64).to(device, non_blocking=True) if ragged else None
            y = self._forward(x, lengths, amp)
            for k, ((r, _), w) in enumerate(zip(batch, ws)):
                if outs[r] is None:
                    outs[r] = torch.empty(plans[r][-1].keep_to, y.shape[2], device=device, dtype=y.dtype)
                outs[r][w.keep_from:w.keep_to].copy_(y[k, w.keep_from - w.first:w.keep_to - w.first])
        return outs


class Transcript(NamedTuple):
    """text: the best hypothesis; words: its align.Words with global times (None without times=True); word_confidence: one
    float per Word (None without confidence=); frames: encoder frames of the recording (with Transcriber(vad=...): the frames
    decoded, those of its speech islands); seconds: its duration (mel frames x the front end's hop)."""
    text: str
    words: Optional[List[Word]]
    word_confidence: Optional[List[float]]
    frames: int
    seconds: float


class Aligned(NamedTuple):
    """words: the transcript's align.Words with global times ([] when the text does not fit the frames); score: the sum over the
    frames of the log-probability of the aligned symbol (-inf when it does not fit); ok: it fits; frames, seconds: as Transcript."""
    words: List[Word]
    score: float
    ok: bool
    frames: int
    seconds: float


class Segmented(NamedTuple):
    """segments: one align.Segment per utterance, in the order given ([] when they do not fit the frames); score, ok, frames,
    seconds: as Aligned (the score counts the wildcard frames at the log-probability of their most likely symbol)."""
    segments: List[Segment]
    score: float
    ok: bool
    frames: int
    seconds: float


class Utterance(NamedTuple):
    """A run of aligned words cut out for training: start / end in seconds, the words [first_word, last_word] of the list it was
    cut from joined by a space, and the mean of their scores weighted by their frames."""
    start: float
    end: float
    text: str
    score: float
    first_word: int
    last_word: int                       # inclusive


def cut_utterances(words: Sequence[Word], max_seconds: float, min_gap_seconds: float) -> List[Utterance]:
    """Cut the aligned words of a recording into utterances (host arithmetic, for corpus building).
    1. Split wherever next.start - prev.end >= min_gap_seconds.
    2. Split any piece longer than max_seconds (last end - first start) at its largest internal gap, the earliest of equal
       ones; repeat until every piece fits or is a single word (a single word longer than max_seconds stands as it is).
    The pieces are returned in order; together they hold every word once."""
    for name, v in (("max_seconds", max_seconds), ("min_gap_seconds", min_gap_seconds)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v <= 0:
            raise ValueError(f"cut_utterances: {name} must be a positive finite number of seconds, got {v!r}")
    words = list(words)
    pieces, first = [], 0
    for i in range(1, len(words) + 1):
        if i == len(words) or words[i].start - words[i - 1].end >= min_gap_seconds:
            pieces.append((first, i - 1))
            first = i
    out: List[Utterance] = []
    stack = pieces[::-1] if words else []
    while stack:
        lo, hi = stack.pop()
        if hi > lo and words[hi].end - words[lo].start > max_seconds:
            gaps = [words[i + 1].start - words[i].end for i in range(lo, hi)]
            cut = lo + gaps.index(max(gaps))                     # index() takes the earliest of equal gaps
            stack += [(cut + 1, hi), (lo, cut)]
            continue
        frames = [w.end_frame - w.start_frame for w in words[lo:hi + 1]]
        total = sum(frames)
        score = sum(w.score * f for w, f in zip(words[lo:hi + 1], frames)) / total if total > 0 else -math.inf
        out.append(Utterance(words[lo].start, words[hi].end, " ".join(w.text for w in words[lo:hi + 1]), score, lo, hi))
    return out


class Transcriber:
    """Offline transcription: a list of recordings in, a list of Transcripts out, in the caller's order.

        tr = Transcriber(model, decoder, frontend, window_seconds=30.0, overlap_seconds=8.0, times=True)
        for t in tr.transcribe(waves, sample_rates=rates): print(t.text)

    model: a Conformer in eval() mode on the HIP device; decoder: a BeamCTCDecoder (its lm and hotwords apply); frontend: a
    ConformerAudioFrontend, then `audios` are waveforms (with sample_rates= whatever the front end takes); None: `audios` are
    log-mel tensors (n_mel, n_i).  Pipeline: front end -> BufferedEncoder.encode -> model.decoder on the stitched frames
    (recordings sorted by length, batches of at most batch_windows) -> the decoder's offline search (text; with times=True
    decoder.words at frame_seconds per encoder frame) -> with confidence=ConfidenceConfig(...) (needs times=True)
    frame_confidence and word_confidence.
    window_seconds, overlap_seconds have NO default: no trained checkpoint was at hand, so no word error rate was measured for
    any choice; 30 s / 8 s is the usual starting point.  They are converted once to mel frames (window_frames: the front end's
    hop, or frame_seconds / 4 per mel frame without one); overlap_seconds is the lower bound of the overlap used.
    batch_windows, graphs: as BufferedEncoder.
    vad=VadConfig(...) (None: off): the voice activity detector runs on the features first (vad.speech_segments, then
    vad.speech_islands) and only the speech islands are encoded: the islands of all recordings go through one
    BufferedEncoder.encode as if they were recordings, each recording's island frames are concatenated for the head and the
    search, and every Word is mapped back to the recording's own time axis.  Transcript.frames is then the number of frames
    decoded, and a recording without speech gives Transcript("", [] or None, [] or None, 0, seconds).  `speech` returns the
    islands.  `align` and `segments` do not use vad: they place a known text on the whole recording.
    Memory: only the encoder is bounded by one batch of windows.  transcribe holds the stitched frames of every recording and,
    per group, a second, padded copy of them (B, T', d) for the decoder head, so twice the stitched output of a group; the head's
    own intermediates, the logits and the search's buffers all grow with the recording's length."""

    def __init__(self, model, decoder: BeamCTCDecoder, frontend: Optional[ConformerAudioFrontend] = None, *,
                 window_seconds: float, overlap_seconds: float, batch_windows: int = 32, graphs: bool = False,
                 times: bool = False, frame_seconds: float = 0.04, confidence: Optional[ConfidenceConfig] = None,
                 vad=None) -> None:
        self.times, self.frame_seconds = times_plan("Transcriber", times, frame_seconds)
        cplan = transcriber_confidence("Transcriber", confidence, 1, self.times)
        self.confidence = None if cplan is None else cplan[0]
        if not isinstance(decoder, BeamCTCDecoder):
            raise ValueError(f"Transcriber: decoder must be a BeamCTCDecoder, got {type(decoder).__name__}")
        if frontend is not None and not isinstance(frontend, ConformerAudioFrontend):
            raise ValueError(f"Transcriber: frontend must be a ConformerAudioFrontend or None, got {type(frontend).__name__}")
        self.mel_seconds = self.frame_seconds / 4 if frontend is None else frontend.hop_length / frontend.sample_rate
        self.window, self.overlap = window_frames(window_seconds, overlap_seconds, self.mel_seconds)
        if isinstance(batch_windows, bool) or not isinstance(batch_windows, int) or batch_windows < 1:
            raise ValueError(f"Transcriber: batch_windows must be a number of windows >= 1, got {batch_windows!r}")
        if not isinstance(graphs, bool):
            raise ValueError(f"Transcriber: graphs must be True or False, got {graphs!r}")
        self.device, _ = lstm_state(model, "Transcriber", 1)
        self.model, self.decoder, self.frontend = model, decoder, frontend
        self.batch_windows = batch_windows
        self.encoder = BufferedEncoder(model.encoder, self.window, self.overlap, batch_windows, graphs)
        self.vad = vad
        if vad is not None:                                      # (the vad module is imported by the objects that use it)
            from .vad import VadConfig
            if not isinstance(vad, VadConfig):
                raise ValueError(f"Transcriber: vad must be a VadConfig or None, got {type(vad).__name__}")
            vad.check(self.mel_seconds, frontend.n_mels if frontend is not None else (vad.band or (0, 1))[1])

    @torch.no_grad()
    def features(self, audios: Sequence[torch.Tensor], sample_rates: Optional[Sequence[int]] = None) -> List[torch.Tensor]:
        """Per recording its log-mel frames (n_mel, n_i): the front end's batch cut back to every recording's own length, or
        `audios` themselves without a front end."""
        if self.frontend is None:
            if sample_rates is not None:
                raise ValueError("Transcriber: sample_rates needs the frontend= (without one the inputs are log-mel frames)")
            return list(audios)
        mels, lengths = self.frontend(audios, sample_rates=sample_rates)
        return [mels[i, :, :n] for i, n in enumerate(lengths.cpu().tolist())]

    @torch.no_grad()
    def decoder_head(self, h: torch.Tensor, lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        """model.decoder on stitched encoder frames h (B, T', d), `lengths` (B) int64 frames per recording: logits (B, T', V)."""
        return self.model.decoder(h, lengths)

    def groups(self, frames: Sequence[int]) -> List[List[int]]:
        """The recordings sorted by encoder frames (longest first, stable), in batches of at most batch_windows."""
        order = sorted(range(len(frames)), key=lambda i: -frames[i])
        return [order[k:k + self.batch_windows] for k in range(0, len(order), self.batch_windows)]

    def _padded_groups(self, hs: Sequence[torch.Tensor]):
        """The encoder frames hs (one (T', d) tensor per recording) in `groups`: per group (group, frames of each, their frames
        zero-padded to the longest (len(group), T', d), the frames as `lengths` (len(group)) int64 on the device)."""
        for group in self.groups([h.shape[0] for h in hs]):
            n = [hs[i].shape[0] for i in group]
            h = hs[group[0]].new_zeros(len(group), n[0], hs[group[0]].shape[1])
            for k, i in enumerate(group):
                h[k, :n[k]] = hs[i]
            yield group, n, h, torch.tensor(n, dtype=torch.int64).to(self.device, non_blocking=True)

    @torch.no_grad()
    def transcribe(self, audios: Sequence[torch.Tensor], sample_rates: Optional[Sequence[int]] = None, hotwords=None,
                   hotword_weight=None) -> List[Transcript]:
        """audios: waveforms as the front end takes them (sample_rates: their rates, None: all at the front end's own), or log-mel
        tensors (n_mel, n_i) without a front end; every recording needs at least 7 mel frames.  One Transcript per recording, in
        the caller's order.  Synchronises (the texts are read back).
        hotwords: one entry per recording (None: the decoder's own list, () or []: none, a Hotwords or phrases), hotword_weight:
        one float or one per recording (None: the decoder's) -- BeamCTCDecoder.__call__, INTEGRATION.md "Per-request hotwords";
        text, words and confidence of a recording all come from the search with its list."""
        lstm_state(self.model, "Transcriber", 1)
        _ambient_autocast("Transcriber")
        if len(audios) == 0:
            return []
        rows = _recording_hotwords(len(audios), hotwords, hotword_weight)
        mels = self.features(audios, sample_rates)
        if self.vad is not None:
            return self._transcribe_islands(mels, rows)
        return self._decode(self.encoder.encode(mels), [m.shape[1] * self.mel_seconds for m in mels], rows)

    def _decode(self, hs: Sequence[torch.Tensor], seconds: Sequence[float], rows=None) -> List[Transcript]:
        """The decoder head, the search and the confidences over encoder frames hs (one (T', d) tensor per recording), in
        groups; one Transcript per recording, in the order given.  rows: None or (hotwords, weights), one entry per recording
        (the same order as hs), which follow their recordings into the groups."""
        out: List[Optional[Transcript]] = [None] * len(hs)
        for group, n, h, lengths in self._padded_groups(hs):
            logits = self.decoder_head(h, lengths)
            kw = {} if rows is None else dict(hotwords=[rows[0][i] for i in group], hotword_weight=[rows[1][i] for i in group])
            texts = self.decoder(logits, lengths, **kw)
            words = self.decoder.words(logits, lengths, self.frame_seconds, **kw) if self.times else [None] * len(group)
            scores = [None] * len(group)
            if self.confidence is not None:
                conf, ids = frame_confidence(logits, lengths, self.confidence)
                scores = word_confidence(words, conf, ids, self.decoder.blank_id, lengths, self.confidence)
            for k, i in enumerate(group):
                out[i] = Transcript(texts[k], words[k], scores[k], n[k], seconds[i])
        return out

    def _islands(self, mels: Sequence[torch.Tensor]) -> List[List[Tuple[int, int]]]:
        """Per recording its speech islands in mel frames: vad.speech_segments, then vad.speech_islands."""
        from . import vad as _vad
        p = self.vad.check(self.mel_seconds, int(mels[0].shape[0]))
        for r, m in enumerate(mels):
            if m.shape[1] < MIN_MEL_FRAMES:
                raise ValueError(f"Transcriber: recording {r} has {m.shape[1]} mel frames, the least is {MIN_MEL_FRAMES}")
        segments = _vad.speech_segments(mels, config=self.vad, mel_seconds=self.mel_seconds)
        return [_vad.speech_islands(s, int(m.shape[1]), p.pad_before, p.pad_after, p.min_gap) for s, m in zip(segments, mels)]

    @torch.no_grad()
    def speech(self, audios: Sequence[torch.Tensor], sample_rates: Optional[Sequence[int]] = None) -> List[List[Tuple[float, float]]]:
        """Per recording the speech islands transcribe would encode, as (start, end) in seconds.  Needs vad=.  Synchronises."""
        if self.vad is None:
            raise ValueError("Transcriber.speech: this Transcriber was made without vad=")
        if len(audios) == 0:
            return []
        mels = [m if m.is_cuda else m.to(self.device) for m in self.features(audios, sample_rates)]
        return [[(a * self.mel_seconds, b * self.mel_seconds) for a, b in isl] for isl in self._islands(mels)]

    def _transcribe_islands(self, mels: Sequence[torch.Tensor], rows=None) -> List[Transcript]:
        """transcribe with vad=: the islands of all recordings through ONE BufferedEncoder.encode as if they were recordings,
        per recording their encoder frames concatenated, _decode over the concatenations, and every Word mapped back to the
        recording's own time axis: frame c of the concatenation that lies j frames into the island (a, b) is the recording's
        frame a / 4 + j; a word's end is the mapped last frame + 1."""
        mels = [m if m.is_cuda else m.to(self.device) for m in mels]
        seconds = [m.shape[1] * self.mel_seconds for m in mels]
        islands = self._islands(mels)
        pieces = [(r, a, b) for r, isl in enumerate(islands) for a, b in isl]
        encoded = self.encoder.encode([mels[r][:, a:b] for r, a, b in pieces]) if pieces else []
        spoken = [r for r, isl in enumerate(islands) if isl]
        mine = {r: [h for h, (r2, _, _) in zip(encoded, pieces) if r2 == r] for r in spoken}
        decoded = self._decode([torch.cat(mine[r]) for r in spoken], [seconds[r] for r in spoken],
                               None if rows is None else ([rows[0][r] for r in spoken], [rows[1][r] for r in spoken]))
        out = [Transcript("", [] if self.times else None, [] if self.confidence is not None else None, 0, s) for s in seconds]
        fs = self.frame_seconds
        for r, t in zip(spoken, decoded):
            if t.words is not None:
                to_global: List[int] = []                        # frame of the concatenation -> frame of the recording
                for (a, _), h in zip(islands[r], mine[r]):
                    to_global += range(a // 4, a // 4 + h.shape[0])
                spans = [(to_global[w.start_frame], to_global[w.end_frame - 1] + 1) for w in t.words]
                t = t._replace(words=[Word(w.text, a, b, a * fs, b * fs, w.score) for w, (a, b) in zip(t.words, spans)])
            out[r] = t
        return out

    def _group_logits(self, audios: Sequence[torch.Tensor], sample_rates: Optional[Sequence[int]]):
        """transcribe's pipeline up to the logits: per group of recordings (group, frames of each, their seconds, logits, lengths)"""
        mels = self.features(audios, sample_rates)
        for group, n, h, lengths in self._padded_groups(self.encoder.encode(mels)):
            yield group, n, [mels[i].shape[1] * self.mel_seconds for i in group], self.decoder_head(h, lengths), lengths

    @torch.no_grad()
    def align(self, audios: Sequence[torch.Tensor], texts: Sequence, sample_rates: Optional[Sequence[int]] = None,
              wildcard_token: Optional[str] = None, wildcard_penalty: Optional[float] = None) -> List[Aligned]:
        """Forced alignment of whole recordings: `texts` holds one transcript per recording, strings or token-id sequences as
        CTCAligner takes them.  Same pipeline as transcribe up to the logits (front end, BufferedEncoder.encode, decoder_head on
        the stitched frames in the same groups), then CTCAligner.from_decoder(decoder, frame_seconds) with long=True: no limit
        on the recording's length but the workspace (align.ctc_forced_align_long).  One Aligned per recording, in the caller's
        order.  Synchronises (the words are read back).
        wildcard_token, wildcard_penalty: CTCAligner's, for a transcript that skips audio (a wildcard where it does)."""
        lstm_state(self.model, "Transcriber", 1)
        _ambient_autocast("Transcriber")
        if isinstance(texts, str) or len(texts) != len(audios):
            raise ValueError(f"Transcriber.align: one text per recording, got {len(audios)} recordings and "
                             f"{'a single string' if isinstance(texts, str) else f'{len(texts)} texts'}")
        if len(audios) == 0:
            return []
        aligner = CTCAligner.from_decoder(self.decoder, self.frame_seconds, wildcard_token, wildcard_penalty)
        targets = [aligner._ids(t) for t in texts]                   # refuses a bad text before anything runs
        out: List[Optional[Aligned]] = [None] * len(audios)
        for group, n, seconds, logits, lengths in self._group_logits(audios, sample_rates):
            ids, al = aligner.align(logits, [targets[i] for i in group], lengths, long=True)
            words = aligner.words(ids, al)
            ok, score = al.ok.cpu().tolist(), al.score.cpu().tolist()
            for k, i in enumerate(group):
                out[i] = Aligned(words[k], score[k], bool(ok[k]), n[k], seconds[k])
        return out

    @torch.no_grad()
    def spot(self, audios: Sequence[torch.Tensor], keywords, sample_rates: Optional[Sequence[int]] = None) -> List[list]:
        """Keyword spotting over whole recordings (INTEGRATION.md "Keyword spotting"): `keywords` is a kws.Keywords.  Same
        pipeline as transcribe up to the logits, as `align`; then kws.spot_keywords on every group's logits.  Per recording,
        in the caller's order, its kws.Detections sorted by (end_frame, keyword), times in seconds of the recording at
        frame_seconds per encoder frame.  Does not use vad.  Synchronises."""
        from . import kws as _kws                                # (imported by the objects that use it)
        lstm_state(self.model, "Transcriber", 1)
        _ambient_autocast("Transcriber")
        if not isinstance(keywords, _kws.Keywords):
            raise ValueError(f"Transcriber.spot: keywords must be a kws.Keywords, got {type(keywords).__name__}")
        if keywords.blank_id != self.decoder.blank_id:
            raise ValueError(f"Transcriber.spot: the keywords' blank is {keywords.blank_id}, the decoder's {self.decoder.blank_id}")
        out: List[Optional[list]] = [None] * len(audios)
        if len(audios) == 0:
            return out
        for group, _, _, logits, lengths in self._group_logits(audios, sample_rates):
            found = _kws.spot_keywords(logits, keywords, lengths, self.frame_seconds)
            for k, i in enumerate(group):
                out[i] = found[k]
        return out

    @torch.no_grad()
    def segments(self, audios: Sequence[torch.Tensor], utterance_lists: Sequence[Sequence], wildcard_penalty: float,
                 sample_rates: Optional[Sequence[int]] = None, ends: bool = True) -> List[Segmented]:
        """Locate utterances in whole recordings: `utterance_lists` holds per recording the texts or token-id sequences it
        contains somewhere, in spoken order; the audio in front of, between and behind them is absorbed by wildcards at
        `wildcard_penalty` logit units per frame (CTCAligner.segments; ends=False: the recording starts and ends with the
        utterances).  The pipeline and the groups of `align`, the long form.  One Segmented per recording, in the caller's
        order.  Synchronises."""
        lstm_state(self.model, "Transcriber", 1)
        _ambient_autocast("Transcriber")
        if isinstance(utterance_lists, str) or len(utterance_lists) != len(audios) or \
                any(isinstance(u, str) for u in utterance_lists):
            raise ValueError(f"Transcriber.segments: one LIST of utterances per recording, got {len(audios)} recordings and "
                             f"{utterance_lists!r}"[:300])
        aligner = CTCAligner.from_decoder(self.decoder, self.frame_seconds, None, wildcard_penalty)
        if aligner.wildcard_penalty is None:
            raise ValueError("Transcriber.segments: wildcard_penalty has no default (it depends on the model's posteriors)")
        if len(audios) == 0:
            return []
        built = [aligner.segment_targets(u, ends) for u in utterance_lists]      # refuses a bad utterance before anything runs
        out: List[Optional[Segmented]] = [None] * len(audios)
        for group, n, seconds, logits, lengths in self._group_logits(audios, sample_rates):
            ids, al = aligner.align(logits, [built[i][0] for i in group], lengths, long=True)
            segs = aligner.segments_of([utterance_lists[i] for i in group], ids, [built[i][1] for i in group], al)
            ok, score = al.ok.cpu().tolist(), al.score.cpu().tolist()
            for k, i in enumerate(group):
                out[i] = Segmented(segs[k], score[k], bool(ok[k]), n[k], seconds[k])
        return out
