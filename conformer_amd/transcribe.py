"""Streaming transcription: mel chunks in, interim and final transcripts out (INTEGRATION.md "Streaming (resumable)
search").

StreamingTranscriber joins the chunked encoder (StreamingEncoder, cached K/V and depthwise state), the decoder with its LSTM
state carried across chunks (ops.lstm_forward(state=...): any chunking equals one call bit for bit) and the resumable beam
search of a BeamCTCDecoder (BeamCTCStream: any chunking equals one-shot decoding bit for bit).  Per chunk: encoder step ->
LSTM layers -> Swish + BatchNorm (running statistics) -> vocabulary Linear on the new frames -> beam step.  All utterances of
the batch advance in lockstep, as in StreamingEncoder; there are no ragged stream ends here.  Everything runs on the gfx950
kernels; the model must be in eval mode on the HIP device.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Tuple

import torch

from . import ops
from .align import Word
from .confidence import ConfidenceConfig, StreamingConfidence, transcriber_confidence
from ._slot_state import positive_seconds
from .decode import BeamCTCDecoder, BeamCTCStream, _flag
from .stream_frontend import StreamingAudioFrontend
from .streaming import StreamingEncoder, encoder_frames, ring_plan


@torch.no_grad()
def decode_frames(model, state, enc: torch.Tensor, lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The decoder (Decoder.fused in eval mode) on new encoder frames (B, k, d) with the LSTM state `state` ([(h, c)] per
    layer, (B, H) each) carried; `lengths` (B) int64 on the device: frames per utterance (None: all k)."""
    dec = model.decoder
    h = enc.float() if enc.dtype != torch.float32 else enc
    for k, st in enumerate(state):
        w_ih, w_hh = getattr(dec.lstm, f"weight_ih_l{k}"), getattr(dec.lstm, f"weight_hh_l{k}")
        b_ih, b_hh = getattr(dec.lstm, f"bias_ih_l{k}"), getattr(dec.lstm, f"bias_hh_l{k}")
        bias = dec._packs.get(f"bias{k}", (b_ih, b_hh), lambda: (b_ih + b_hh).detach().contiguous())
        h = ops.lstm_forward(h, w_ih.detach(), w_hh.detach(), bias, lengths, state=st)
    n = dec.norm
    z = ops.swish_bn_eval(h, n.running_mean, n.running_var, n.weight.detach(), n.bias.detach(), n.eps)
    return ops.linear(z, dec.linear.weight.detach(), dec.linear.bias.detach())


def search_plan(who: str, max_mel_frames, left_context, max_chunk_mel_frames, max_pending):
    """The transcribers' sizing of the beam search, checked on the host before anything else: None (the search ends with
    max_mel_frames) or (max_pending, k_cap), k_cap = ring_plan's encoder frames per step."""
    if max_mel_frames is None and left_context is None:
        raise ValueError(f"{who}: max_mel_frames=None (a stream without an end) needs left_context")
    if max_pending is None:
        if max_mel_frames is None:
            raise ValueError(f"{who}: max_mel_frames=None (a stream without an end) needs max_pending: without it the beam "
                             "search's buffers are sized by the stream's length")
        return None
    if left_context is None or max_chunk_mel_frames is None:
        missing = "left_context" if left_context is None else "max_chunk_mel_frames"
        raise ValueError(f"{who}: max_pending needs {missing} (the search's tree is sized for the largest step of a windowed "
                         "stream)")
    if int(max_pending) < 1:
        raise ValueError(f"{who}: max_pending must be >= 1 token, got {max_pending}")
    return int(max_pending), ring_plan(left_context, max_chunk_mel_frames)[2]


def times_plan(who: str, times, frame_seconds) -> Tuple[bool, float]:
    """The transcribers' timestamp options, checked on the host before anything else."""
    return _flag(who, "times", times), positive_seconds(who, "frame_seconds", frame_seconds)


def search_stream(decoder: BeamCTCDecoder, plan, batch: int, t_max: Optional[int], device, commit_log: int,
                  times: Tuple[bool, float] = (False, 0.04), hotword_rows: Optional[Tuple[int, int]] = None) -> BeamCTCStream:
    """The transcribers' search for a search_plan: one that ends with the encoder's t_max frames, or a committing one.
    times: a times_plan; (False, ...) makes the stream exactly as before.  hotword_rows: (max_phrases, max_code_points) reserved
    per utterance for per-request hotwords; None makes the stream exactly as before."""
    kw = dict(times=True, frame_seconds=times[1]) if times[0] else {}
    if hotword_rows is not None:
        kw["hotword_rows"] = hotword_rows
    if plan is None:
        return decoder.stream(batch, t_max, device, **kw)
    return decoder.stream(batch, None, device, max_pending=plan[0], max_chunk_frames=plan[1], commit_log=commit_log, **kw)


def lstm_state(model, who: str, batch: int):
    """Refuses what the streaming transcribers (`who`: the class the message names) cannot run; returns the model's device and
    the zero LSTM state, [(h, c)] per layer, (batch, H) each."""
    if model.training:
        raise RuntimeError(f"{who}: put the model in eval() mode (running BatchNorm statistics, no dropout)")
    dec = model.decoder
    p = next(dec.parameters())
    if not p.is_cuda or p.dtype != torch.float32:
        raise RuntimeError(f"{who}: the model must live on the HIP device in fp32 (no CPU fallback)")
    if not dec._hip_eligible(p):
        raise RuntimeError(f"{who}: the decoder LSTM has no HIP kernel (hidden size % 4 != 0, bidirectional, projected or "
                           "with dropout)")
    H = dec.lstm.hidden_size
    return p.device, [(torch.zeros(batch, H, device=p.device, dtype=torch.float32),
                       torch.zeros(batch, H, device=p.device, dtype=torch.float32)) for _ in range(dec.lstm.num_layers)]


class StreamingTranscriber:
    """model: a Conformer in eval() mode on the HIP device; decoder: the BeamCTCDecoder whose configuration (beam knobs, lm,
    hotwords) the streamed search takes; batch utterances of at most max_mel_frames mel frames.  graphs, check_weights,
    left_context, max_chunk_mel_frames: as StreamingEncoder (without max_pending, max_mel_frames still sizes the beam search's
    buffers; with left_context the encoder no longer allocates by it).
    max_pending=M (tokens; needs left_context): the search commits the prefix that can no longer change after every step
    (INTEGRATION.md "Committed-prefix streaming (max_pending)"), its buffers are sized by M and the largest step alone, and
    max_mel_frames may be None: a stream without an end.  pop_committed() hands out the final tokens as they come.
    times=True: the search records token timestamps (INTEGRATION.md "Beam-search timestamps"): partial_words(), finish_words()
    and, with max_pending, pop_committed_words() return align.Words at frame_seconds per encoder frame.
    audio=StreamingAudioFrontend(frontend, batch, max_chunk_samples): step_audio(samples, flush=False) takes the waveform
    instead of mel frames (INTEGRATION.md "Streaming audio front end"); the transcriber opens every slot of it, reset() again.
    confidence=ConfidenceConfig(...) (needs times=True): every step also keeps the frame confidence of the logits it returns, for
    the last confidence_history frames (INTEGRATION.md "Confidence"); word_confidence(words) gives the Words this object
    returned their confidence.  Without it nothing is launched or allocated.
    hotword_rows=(max_phrases, max_code_points): every utterance may take its own hotword list within those bounds (INTEGRATION.md
    "Per-request hotwords"): set_hotwords(b, ...) after construction or reset(), before the next step.  Without it the object is
    exactly as before."""

    audio: Optional[StreamingAudioFrontend] = None
    confidence: Optional[StreamingConfidence] = None

    def __init__(self, model, decoder: BeamCTCDecoder, batch: int, max_mel_frames: Optional[int], graphs: bool = False,
                 check_weights: bool = True, *, left_context: Optional[int] = None,
                 max_chunk_mel_frames: Optional[int] = None, max_pending: Optional[int] = None,
                 commit_log: int = 4096, times: bool = False, frame_seconds: float = 0.04,
                 audio: Optional[StreamingAudioFrontend] = None, confidence: Optional[ConfidenceConfig] = None,
                 confidence_history: int = 4096, hotword_rows: Optional[Tuple[int, int]] = None) -> None:
        tplan = times_plan("StreamingTranscriber", times, frame_seconds)
        cplan = transcriber_confidence("StreamingTranscriber", confidence, confidence_history, tplan[0])
        plan = search_plan("StreamingTranscriber", max_mel_frames, left_context, max_chunk_mel_frames, max_pending)
        self.B = int(batch)
        if audio is not None:
            if audio.S != self.B:
                raise ValueError(f"StreamingTranscriber: the audio front end has {audio.S} slots, the batch is {self.B}")
            audio.reset()
            for s in range(self.B):
                audio.open(s)
        self.audio = audio
        device, self.state = lstm_state(model, "StreamingTranscriber", self.B)
        self.model = model
        self.encoder = StreamingEncoder(model.encoder, batch, max_mel_frames, graphs=graphs, check_weights=check_weights,
                                        left_context=left_context, max_chunk_mel_frames=max_chunk_mel_frames)
        self.beam = search_stream(decoder, plan, self.B, self.encoder.t_max, device, commit_log, tplan, hotword_rows)
        if cplan is not None:
            self.confidence = StreamingConfidence(self.B, decoder.blank_id, cplan[0], cplan[1], device)

    def set_hotwords(self, b: int, hotwords, hotword_weight: Optional[float] = None) -> None:
        """With hotword_rows=: utterance b's hotword list and weight (BeamCTCStream.set_hotwords), after construction or reset()
        and before the next step.  The lists stay over reset()."""
        self.beam.set_hotwords(b, hotwords, hotword_weight)

    def reset(self) -> None:
        self.encoder.reset()
        if self.confidence is not None:
            self.confidence.reset()
        for h, c in self.state:
            h.zero_()
            c.zero_()
        self.beam.reset()
        if self.audio is not None:
            self.audio.reset()
            for s in range(self.B):
                self.audio.open(s)

    @torch.no_grad()
    def step_audio(self, samples: torch.Tensor, flush: bool = False) -> torch.Tensor:
        """step() from the waveform (needs audio=): samples (B, N) fp32, the next N samples of every utterance (lockstep: N >= 0
        for all; with a front end built with input=, whatever it takes: INTEGRATION.md "Input sample rates"); flush=True with
        the last ones, which completes the frames that reflect the end of the audio.  Returns what step() returns for the mel
        frames the samples complete.  After a flush the text is read with finish(); reset() starts the next utterances.  Every
        refusal raises before anything is enqueued."""
        if self.audio is None:
            raise RuntimeError("StreamingTranscriber: step_audio needs the audio= front end")
        n = samples.shape[1] if isinstance(samples, torch.Tensor) and samples.dim() in (2, 3) else 0
        p = self.audio.plan(samples, [n] * self.B, range(self.B) if flush else ())
        enc = self.encoder
        if enc.left is not None and p.f_max > enc.max_chunk:
            raise ValueError(f"StreamingTranscriber: a step of {p.f_max} mel frames, the ring was sized for "
                             f"max_chunk_mel_frames={enc.max_chunk}")
        if enc.t_max is not None and enc.frames + max(0, encoder_frames(enc.tail_len + p.f_max)) > enc.t_max:
            raise RuntimeError(f"StreamingTranscriber: stream longer than max_mel_frames (T'max = {enc.t_max})")
        mel, _ = self.audio.run(p)
        return self.step(mel)

    @torch.no_grad()
    def decode_frames(self, enc: torch.Tensor) -> torch.Tensor:
        """The decoder (Decoder.fused in eval mode) on the chunk's new encoder frames (B, k, d), the LSTM state carried."""
        return decode_frames(self.model, self.state, enc)

    @torch.no_grad()
    def step(self, mel_chunk: torch.Tensor) -> torch.Tensor:
        """mel_chunk (B, n_mel, Tc): the next log-mel frames.  Returns the logits (B, k, V) of the encoder frames that became
        computable (k may be 0) and advances the beam search over them; nothing synchronises with the host."""
        enc = self.encoder.step(mel_chunk)
        if enc.shape[1] == 0:
            return enc.new_empty(self.B, 0, self.model.decoder.linear.out_features)
        logits = self.decode_frames(enc)
        self.beam.step(logits)
        if self.confidence is not None:
            self.confidence.step(logits)
        return logits

    def word_confidence(self, words: List[List[Word]]) -> List[List[float]]:
        """With confidence=: per utterance the confidence of Words this object returned (partial_words, finish_words,
        pop_committed_words), each over its frames [start_frame, end_frame); nan for a word whose start has left
        confidence_history.  Synchronises."""
        if self.confidence is None:
            raise RuntimeError("StreamingTranscriber.word_confidence: the object was made without confidence=, no frame was "
                               "scored")
        return self.confidence.words(words)

    def partial_text(self) -> List[str]:
        return self.beam.partial_text()

    def pop_committed(self) -> List[List[int]]:
        """With max_pending: per utterance the token ids that became final since the previous pop (BeamCTCStream)."""
        return self.beam.pop_committed()

    def committed_text(self) -> List[str]:
        return self.beam.committed_text()

    def finish(self, decode_func: Optional[Callable[[str], str]] = None) -> List[str]:
        return self.beam.finish(decode_func)

    def pop_committed_words(self) -> List[List[Word]]:
        """With max_pending and times: per utterance the complete words that became final since the previous pop
        (BeamCTCStream.pop_committed_words: the tokens after the last committed delimiter are held back)."""
        return self.beam.pop_committed_words()

    def partial_words(self) -> List[List[Word]]:
        """With times: the words of partial_text()."""
        return self.beam.partial_words()

    def finish_words(self) -> List[List[Word]]:
        """With times: the words of finish(), which this call is in its place."""
        return self.beam.finish_words()
