"""``OfflineRenderer`` — host-side mirror of the reference's offline-render caller.

Follows js/packages/offline-renderer/index.ts:11-186 (``initialize`` option names and defaults
:20-27, the block loop of ``process`` :87-133 which always renders FULL blocks and zero-pads a
short input, ``setCurrentTime`` :179-185) on top of any engine with the ``CRuntime`` surface.
The engine is injected (``engine_factory(sample_rate, block_size) -> CRuntime``) so the same
caller drives the HIP engine in production and the CPU checkers in tests.
"""
from __future__ import annotations

from typing import Any, Callable, Dict, List, Optional, Sequence

import numpy as np


def _is_flac(in_fmt) -> bool:
    """``in_fmt`` 'flac' (or the C-ABI's 4): the inputs are ``FlacChunk`` objects, not arrays."""
    return in_fmt.lower() == "flac" if isinstance(in_fmt, str) else in_fmt == 4


class OfflineRenderer:
    def __init__(self, engine_factory: Callable[[float, int], Any]):
        self._factory = engine_factory
        self._rt: Any = None
        self._listeners: Dict[str, list] = {}

    def initialize(self, num_input_channels: int = 0, num_output_channels: int = 2, sample_rate: float = 44100,
                   block_size: int = 512, virtual_file_system: Optional[Dict[str, np.ndarray]] = None,
                   event_history_blocks: int = 0, capture_history_blocks: int = 0, loudness_meter: bool = False,
                   output_sample_rate: Optional[float] = None, limiter=None, input_sample_rate: Optional[float] = None, noise_shape=None,
                   spectrum: Optional[Dict[str, Any]] = None, qc: Optional[Dict[str, Any]] = None) -> None:
        """``event_history_blocks`` (no counterpart in the reference; 0 = off): engine option of the same name — `scope` and `fft`
        nodes keep a device ring long enough for a relay window of that many blocks, so ``process`` still renders launch sets of
        that size with such a listener attached (engines without ``set_option`` relay after every block anyway).
        ``capture_history_blocks`` (likewise): the same for `capture` and `mc.capture` nodes — a device ring that keeps that many
        blocks of takes and a per-block log from which the blockwise relay places every take at the block where the gate fell.
        ``loudness_meter`` (likewise; off by default): engine option of the same name — every launch set that ``process`` (in engine
        calls of many blocks), ``process_pcm``, ``process_pcm_io``, ``write_wav`` and ``process_wav`` render is metered on the GPU:
        BS.1770 sub-block energies and true peak, read with ``loudness()``.
        ``output_sample_rate`` (likewise; None or ``sample_rate`` itself: off): engine option ``resample_rate`` — the engine renders at
        ``sample_rate`` and ``process`` (whose output buffers then hold the DELIVERED frames: ``ceil(rendered * up / down)`` of them),
        ``process_pcm`` and ``process_pcm_io`` deliver at this rate, converted on the GPU by a windowed-sinc filter whose latency is
        ``resample()['latency_frames']`` output frames; ``write_wav`` and ``process_wav`` write files at this rate with that latency
        taken out. Rendering at 4 x 44100 and delivering 44100 is oversampling. An engine without the option raises ``RuntimeError``.
        ``limiter`` (likewise; None or False: off): ``True`` for the defaults or a dict with any of ``ceiling_dbtp`` (-1), ``gain_db``
        (0), ``lookahead_ms`` (1.5), ``release_ms`` (500) and ``link`` (channels per linked group; 0: all) — engine options ``limiter``
        and ``limiter_*``: a static gain and a look-ahead true-peak limiter on the GPU on everything ``process`` (in engine calls of
        many blocks), ``process_pcm`` and ``process_pcm_io`` deliver, behind the converter and in front of the PCM packing and the
        meter, with a latency of ``limiter()['latency_frames']`` delivered frames; ``write_wav`` and ``process_wav`` take that latency
        out. The delivered sample peak stays under the ceiling; the metered true peak of the output may exceed it slightly (about
        0.1 dB at a look-ahead of one frame, 0.004 dB at 66). An engine without the option raises ``RuntimeError``.
        ``input_sample_rate`` (likewise; None or ``sample_rate`` itself: off): engine option ``input_rate`` — the inputs of ``process``,
        ``process_pcm`` and ``process_pcm_io`` arrive at this rate and are converted to ``sample_rate`` on the GPU by the same
        windowed-sinc filter, with a latency of ``input_resample()['latency_frames']`` ENGINE frames. Frame counts stay in engine
        frames; a call of ``m`` of them consumes ``runtime.input_resample_frames(m)`` input frames from where the last one stopped,
        and inputs that end early are padded with silence. ``process_wav`` then takes files at this rate, with that latency taken
        out. With ``sample_rate`` = 4 x 44100 and both rates 44100, a 44.1 kHz file is processed with fourfold oversampling. An
        engine without the option raises ``RuntimeError``.
        ``noise_shape`` (likewise; None: off): a preset of ``elementary_amd.noise_shape`` ('first', 'second', 'lipshitz5',
        'fweighted9', 'modified_e9') or up to 12 raw coefficients c_1 .. c_K — the s16 / s24 samples of ``process_pcm``,
        ``process_pcm_io``, ``write_wav``, ``write_flac`` and ``process_wav`` come from an error-feedback quantiser on the GPU
        (``Runtime.noise_shape``) behind the limiter, whose error is the dither's shaped by 1 - sum c_k z^-k: out of the 2 - 5 kHz
        region, towards the top of the band. The three psychoacoustic presets are 44.1 kHz designs and raise ``ValueError`` unless the
        delivery rate is 44100 or 48000; raw coefficients are taken at any rate. With ``dither_seed=None`` the shaping runs
        undithered: deterministic, and idle tones are possible. Float delivery is never touched.
        ``spectrum`` (likewise; None: off): a dict of ``size`` (256 .. 4096), and optionally ``hop`` (``size / 4``), ``window``
        ('hann'), ``center`` (False) and either ``bands`` (band rows) or ``mel`` (a count, or a dict of ``n``, ``fmin``, ``fmax``: rows
        of ``elementary_amd.spectrum.mel_bands`` at the delivery rate) — everything ``process`` (in engine calls of many blocks),
        ``process_pcm``, ``process_pcm_io``, ``write_wav``, ``write_flac`` and ``process_wav`` deliver is analysed on the GPU as STFT
        power or band spectra (``Runtime.spectrum``), behind the converter and the limiter and before any quantisation; read with
        ``spectrogram()``. An engine without the calls raises ``RuntimeError``."""
        self.num_in = int(num_input_channels)
        self.num_out = int(num_output_channels)
        self.block_size = int(block_size)
        self.sample_rate = float(sample_rate)
        self._rt = self._factory(self.sample_rate, self.block_size)
        if event_history_blocks and hasattr(self._rt, "set_option"):
            self._rt.set_option("event_history_blocks", int(event_history_blocks))
        if capture_history_blocks and hasattr(self._rt, "set_option"):
            self._rt.set_option("capture_history_blocks", int(capture_history_blocks))
        self._loudness = bool(loudness_meter)
        if self._loudness:
            self._rt.set_option("loudness_meter", 1)
        self.output_sample_rate = self.sample_rate
        self._resample = output_sample_rate is not None and float(output_sample_rate) != self.sample_rate
        if self._resample:
            if not hasattr(self._rt, "set_option") or not hasattr(self._rt, "resample_read"):
                raise RuntimeError("this engine cannot deliver at another sample rate (option resample_rate)")
            try:
                self._rt.set_option("resample_rate", float(output_sample_rate))
            except RuntimeError as e:
                raise RuntimeError(f"this engine cannot deliver {self.sample_rate:g} Hz renders at {float(output_sample_rate):g} Hz") from e
            self.output_sample_rate = float(output_sample_rate)
        self._limiter = limiter is not None and limiter is not False
        if self._limiter:
            if not hasattr(self._rt, "set_option") or not hasattr(self._rt, "limiter_read"):
                raise RuntimeError("this engine has no limiter (option limiter)")
            params = {} if limiter is True else dict(limiter)
            unknown = set(params) - {"ceiling_dbtp", "gain_db", "lookahead_ms", "release_ms", "link"}
            if unknown:
                raise ValueError(f"unknown limiter parameters: {sorted(unknown)}")
            try:
                for k, v in params.items():
                    self._rt.set_option("limiter_" + k, float(v))
                self._rt.set_option("limiter", 1)
            except RuntimeError as e:
                raise RuntimeError(f"this engine cannot limit with {params} at {self.output_sample_rate:g} Hz") from e
        self.input_sample_rate = self.sample_rate
        self._inres = input_sample_rate is not None and float(input_sample_rate) != self.sample_rate
        if self._inres:
            if not hasattr(self._rt, "set_option") or not hasattr(self._rt, "input_resample_read"):
                raise RuntimeError("this engine cannot take inputs at another sample rate (option input_rate)")
            try:
                self._rt.set_option("input_rate", float(input_sample_rate))
            except RuntimeError as e:
                raise RuntimeError(f"this engine cannot take {float(input_sample_rate):g} Hz inputs at {self.sample_rate:g} Hz") from e
            self.input_sample_rate = float(input_sample_rate)
        from . import noise_shape as _ns
        shape = _ns.resolve(noise_shape, self.output_sample_rate)
        self._noise_shape = shape is not None
        if self._noise_shape:
            if not hasattr(self._rt, "noise_shape"):
                raise RuntimeError("this engine has no noise shaping (Runtime.noise_shape)")
            try:
                self._rt.noise_shape(shape)
            except RuntimeError as e:
                raise ValueError(f"this engine refuses the noise-shaping coefficients {shape}") from e
        self._spectrum = spectrum is not None
        if self._spectrum:
            if not hasattr(self._rt, "spectrum") or not hasattr(self._rt, "spectrum_read"):
                raise RuntimeError("this engine has no spectrum analyser (Runtime.spectrum)")
            params = dict(spectrum)
            unknown = set(params) - {"size", "hop", "window", "center", "bands", "mel"}
            if unknown or "size" not in params or ("bands" in params and "mel" in params):
                raise ValueError(f"spectrum: 'size' and any of hop, window, center and one of bands / mel; got {sorted(params)}")
            bands = params.get("bands")
            if params.get("mel") is not None:
                from . import spectrum as _sp
                mel = params["mel"] if isinstance(params["mel"], dict) else {"n": int(params["mel"])}
                bands = _sp.mel_bands(self.output_sample_rate, int(params["size"]), int(mel["n"]), float(mel.get("fmin", 0.0)), mel.get("fmax"))
            try:
                self._rt.spectrum(int(params["size"]), params.get("hop"), params.get("window", "hann"), bands, bool(params.get("center", False)))
            except RuntimeError as e:
                raise ValueError(f"this engine refuses the spectrum spec (size {params['size']}, hop {params.get('hop')})") from e
        self._spectrum_parts = []
        # ``qc`` (likewise; None: off): the inspector's spec (``Runtime.qc``: silence_level, clip_level, clip_run, dropout_frames, bucket,
        # pairs, skip, limit) — everything ``process`` (in engine calls of many blocks), ``process_pcm``, ``process_pcm_io``,
        # ``process_flac`` and the file wrappers deliver is inspected on the GPU; read with ``qc()``. Not covered: the device-resident
        # ``process_blocks``, and ``process`` block by block outside the host-block path.
        self._qc = None if qc is None else dict(qc)
        self._qc_overview = []
        if self._qc is not None:
            if not hasattr(self._rt, "qc") or not hasattr(self._rt, "qc_read"):
                raise RuntimeError("this engine has no inspector (Runtime.qc)")
            try:
                self._rt.qc(self._qc)
            except RuntimeError as e:
                raise ValueError(f"this engine refuses the qc spec {self._qc}") from e
        self._time = 0
        self._lanes: Dict[int, list] = {}
        for k, v in (virtual_file_system or {}).items():
            self._rt.add_shared_resource(k, v)

    def automate(self, lanes: Dict[int, Sequence], unit: str = "frames") -> None:
        """Breakpoint automation (no counterpart in the reference): ``{channel: [(frame_or_seconds, value, "hold" | "linear"), ...]}``
        binds each list — sorted by time; ``elementary_amd.automation`` has ``ramp``, ``steps`` and the value rule — as a lane to engine
        input channel ``channel`` (``Runtime.automation``), which ``el.in({"channel": channel})`` reads like any input. The lanes'
        channels count into the engine's inputs behind the ``num_input_channels`` the caller supplies, so ``channel`` lies in
        ``num_input_channels .. 31``; an empty list clears a lane. ``unit`` "seconds": times convert with
        ``round(seconds * sample_rate)`` (the engine's rate, also with ``input_sample_rate`` set: lanes are not converted). The lanes are
        expanded on the GPU at the renderer's running sample time, so ``process``, ``process_pcm``, ``process_pcm_io``, ``write_wav``,
        ``write_flac`` and ``process_wav`` need nothing more. A lane the engine refuses raises ``ValueError`` and changes nothing."""
        from . import automation as _au
        if unit not in ("frames", "seconds"):
            raise ValueError(f"unit is 'frames' or 'seconds', got {unit!r}")
        if not hasattr(self._rt, "automation"):
            raise RuntimeError("this engine has no automation lanes (Runtime.automation)")
        for channel, points in lanes.items():
            ch = int(channel)
            if not self.num_in <= ch < _au.MAX_CHANNELS:
                raise ValueError(f"lane channel {ch}: lanes bind to channels {self.num_in} .. {_au.MAX_CHANNELS - 1}, behind the {self.num_in} supplied inputs")
            pts = _au.normalise(_au.to_frames(points, self.sample_rate) if unit == "seconds" else points)
            try:
                self._rt.automation(ch, pts)
            except RuntimeError as e:
                raise ValueError(f"this engine refuses the lane of channel {ch}") from e
            if pts:
                self._lanes[ch] = pts
            else:
                self._lanes.pop(ch, None)

    @property
    def runtime(self) -> Any:
        return self._rt

    def on(self, kind: str, callback) -> None:
        """EventEmitter.on of the reference renderer (index.ts:14): 'meter', 'snapshot', ..."""
        self._listeners.setdefault(kind, []).append(callback)

    def render(self, *roots: Any) -> Dict[str, Any]:
        stats = self._rt.render(*roots)
        if stats["result"] != 0:
            raise RuntimeError(f"render failed: code {stats['result']}")
        return stats

    def create_ref(self, kind: str, props: Dict[str, Any], children: Sequence[Any]):
        return self._rt.renderer.create_ref(kind, props, children)

    def process(self, inputs: Sequence[np.ndarray], outputs: Sequence[np.ndarray]) -> None:
        """The reference's block loop. With ``initialize(limiter=...)`` the buffers hold the LIMITED frames, the limiter's latency
        included: frame n is the gained and limited render at n - latency_frames, silence first (renders longer than one block only;
        an engine without ``process_blocks_host`` cannot limit)."""
        if len(inputs) != self.num_in:
            raise ValueError(f"Invalid input data; expected {self.num_in} buffers.")
        if len(outputs) != self.num_out:
            raise ValueError(f"Invalid output data; expected {self.num_out} buffers.")
        if self.num_out == 0:
            return
        bs = self.block_size
        total = len(outputs[0])
        host_batch = getattr(self._rt, "process_blocks_host", None)
        window = getattr(self._rt, "event_window_blocks", None)
        if self._resample:
            # the output buffers hold DELIVERED frames: render the inputs' length, or — without inputs — what fills the buffers
            info = self._rt.resample_read()
            total = max([len(b) for b in inputs], default=-((-total * info["down"]) // info["up"]))
            if getattr(self, "_inres", False) and self.num_in:      # (the inputs' length in ENGINE frames)
                iinfo = self._rt.input_resample_read()
                total = -((-total * iinfo["up"]) // iinfo["down"])
        inres = getattr(self, "_inres", False) and self.num_in > 0
        icur = 0                                     # input frames consumed so far (option input_rate: not the engine's count)
        lanes = bool(getattr(self, "_lanes", None))     # automate(): lanes live in the host-buffer calls only
        if host_batch is not None and window is not None and any(self._listeners.values()) and (total > bs or self._resample or self._limiter or inres or lanes):
            # listeners to serve: the reference relays events after EVERY block (index.ts:112-122). The engine keeps per-block readout
            # logs, so the block loop still runs as launch sets — `event_window_blocks()` blocks per engine call (1024 with meters and
            # snapshots only, fewer with a scope ring, one with a capture node made without history) — and the BLOCKWISE relay after each call hands the
            # listeners every block's events in block order, as the per-block loop would have
            w = max(1, int(window())) * bs
            at = 0                                   # delivered frames so far
            for k in range(0, total, w):
                m = min(w, total - k)
                x = None
                if self.num_in:
                    x, icur = self._pull(inputs, icur, m)
                y = host_batch(x, self.num_out, m, sample_time=self._time)
                self._time += ((m + bs - 1) // bs) * bs
                for kind, payload in self._rt.process_queued_events(blockwise=True):
                    for cb in self._listeners.get(kind, []):
                        cb(payload)
                for i, buf in enumerate(outputs):
                    mm = min(y.shape[1], len(buf) - at)
                    if mm > 0:
                        buf[at:at + mm] = y[i, :mm]
                at += y.shape[1]
            return
        if host_batch is not None and not any(self._listeners.values()) and (total > bs or self._resample or self._limiter or inres or lanes):
            # no event listeners to serve between blocks: the whole block loop in one engine call
            # (elemhip_process_blocks_host: launch sets staged through pinned double buffers); the event queues are drained
            # once afterwards, as the per-block loop's relay (index.ts:118-122) would have kept them drained — a listener
            # attached later must not find a capture / scope ring that overran during this render
            x = None
            if self.num_in:
                x, icur = self._pull(inputs, icur, total)
            y = host_batch(x, self.num_out, total, sample_time=self._time)
            self._time += ((total + bs - 1) // bs) * bs
            self._rt.process_queued_events()
            for i, buf in enumerate(outputs):
                m = min(y.shape[1], len(buf))
                buf[:m] = y[i, :m]
            return
        if self._resample:
            raise RuntimeError("this engine cannot deliver at another sample rate (no process_blocks_host)")
        if self._limiter and host_batch is None:
            raise RuntimeError("this engine cannot limit (no process_blocks_host)")
        if inres:
            raise RuntimeError("this engine cannot take inputs at another sample rate (no process_blocks_host)")
        if lanes:
            raise RuntimeError("automation lanes need process_blocks_host, without event listeners or with event_window_blocks")
        for k in range(0, total, bs):
            block_in = None
            if self.num_in:
                block_in = np.zeros((self.num_in, bs), dtype=np.float32)
                for i, buf in enumerate(inputs):
                    seg = np.asarray(buf[k:k + bs], dtype=np.float32)
                    block_in[i, :len(seg)] = seg
            out = self._rt.process(block_in, self.num_out, bs, sample_time=self._time)
            self._time += bs
            for kind, payload in self._rt.process_queued_events():     # index.ts:118-122: relay events after every block
                for cb in self._listeners.get(kind, []):
                    cb(payload)
            for i, buf in enumerate(outputs):
                m = min(bs, len(buf) - k)
                if m > 0:
                    buf[k:k + m] = out[i, :m]

    def _pull(self, inputs, cursor: int, m: int):
        """The planar inputs of an engine call of ``m`` frames, from input frame ``cursor`` on, padded with silence: ``m`` frames, or
        — ``initialize(input_sample_rate=...)`` — the ``input_resample_frames(m)`` frames the call consumes. Returns them and the
        cursor behind them."""
        ni = self._rt.input_resample_frames(m) if getattr(self, "_inres", False) else m
        x = np.zeros((self.num_in, ni), dtype=np.float32)
        for i, buf in enumerate(inputs):
            seg = np.asarray(buf[cursor:cursor + ni], dtype=np.float32)
            x[i, :len(seg)] = seg
        return x, cursor + ni

    def process_pcm(self, inputs: Sequence[np.ndarray], num_streams: int, channels_per_stream: int, num_frames: int, fmt="s16",
                    dither_seed: Optional[int] = None, want_float: bool = False, sample_time: Optional[int] = None):
        """``process`` delivered as interleaved PCM packed on the GPU (``Runtime.process_blocks_pcm``, same arguments apart from the
        engine): returns ``(streams, stats, planar)``. With listeners attached the render walks ``event_window_blocks()`` windows
        with the blockwise relay between them, as ``process`` does; every window is packed at its absolute time, so the bytes are
        those of one call. With ``initialize(limiter=...)`` the streams hold the limited frames with the limiter's latency in them:
        frame n is the limited render at n - latency_frames."""
        if len(inputs) != self.num_in:
            raise ValueError(f"Invalid input data; expected {self.num_in} buffers.")
        if int(num_streams) * int(channels_per_stream) != self.num_out:
            raise ValueError(f"Invalid stream layout; expected {self.num_out} channels in all.")
        pcm = getattr(self._rt, "process_blocks_pcm", None)
        if pcm is None:
            raise RuntimeError("this engine has no PCM delivery (process_blocks_pcm)")
        bs, total = self.block_size, int(num_frames)
        if sample_time is not None:
            self._time = int(sample_time)
        listening = any(self._listeners.values()) and hasattr(self._rt, "event_window_blocks")
        w = max(1, int(self._rt.event_window_blocks())) * bs if listening else max(total, 1)
        parts = []
        icur = 0
        for k in range(0, max(total, 1), w):
            m = min(w, total - k)
            x = None
            if self.num_in:
                x, icur = self._pull(inputs, icur, m)
            parts.append(pcm(x, num_streams, channels_per_stream, m, fmt, dither_seed=dither_seed, want_float=want_float, sample_time=self._time))
            self._time += ((m + bs - 1) // bs) * bs
            events = self._rt.process_queued_events(blockwise=True) if listening else self._rt.process_queued_events()
            for kind, payload in events:
                for cb in self._listeners.get(kind, []):
                    cb(payload)
        if len(parts) == 1:
            return parts[0]
        streams = [np.concatenate([p[0][s] for p in parts]) for s in range(int(num_streams))]
        stats = {"peak": np.max([p[1]["peak"] for p in parts], axis=0), "over": np.sum([p[1]["over"] for p in parts], axis=0, dtype=np.uint64),
                 "nonfinite": np.sum([p[1]["nonfinite"] for p in parts], axis=0, dtype=np.uint64)}
        planar = np.concatenate([p[2] for p in parts], axis=1) if want_float else None
        return streams, stats, planar

    # -- option flac_in_md5: the STREAMINFO MD5 of FLAC inputs, computed on the GPU and compared here ------------------------------
    def verify_begin(self) -> None:
        """A programme of FLAC inputs that is to be verified starts: option ``flac_in_md5`` on, every input slot reset."""
        self._rt.set_option("flac_in_md5", 1)
        self._rt.flac_in_md5_reset()

    def verify_end(self, expected: Sequence[Optional[bytes]], output=None) -> List[str]:
        """The programme's verdicts, one per input stream: ``expected[s]`` is the MD5 input ``s`` announces (``FlacReader.md5``;
        None or sixteen zeros: none). 'ok', 'absent' (nothing announced: not a mismatch), 'incomplete' (the render ended before the
        stream did, started behind its first sample or skipped a part) or 'mismatch' — which raises ``FlacMd5Mismatch`` for the
        first such input, with ``output`` (what was written, left in place) named in it. Also kept as ``self.input_md5``."""
        from .runtime import FlacMd5Mismatch, flac_md5_verdict
        got = self._rt.flac_in_md5()
        verdicts = []
        for s, exp in enumerate(expected):
            exp = bytes(16) if exp is None else bytes(exp)
            have = s < len(got["state"])
            verdicts.append(flac_md5_verdict(got["state"][s] if have else 0, got["md5"][s] if have else bytes(16), exp))
        self.input_md5 = verdicts
        for s, v in enumerate(verdicts):
            if v == "mismatch":
                err = FlacMd5Mismatch(s, expected[s], got["md5"][s], output)
                err.input_md5 = verdicts
                raise err
        return verdicts

    def process_flac(self, inputs: Sequence[np.ndarray], num_streams: int, channels_per_stream: int, num_frames: int, bits: int = 16,
                     dither_seed: Optional[int] = None, sample_time: Optional[int] = None, drop: int = 0, take: Optional[int] = None, in_fmt=None,
                     verify_input: bool = False):
        """``process_pcm`` delivered as FLAC frames encoded on the GPU (``Runtime.process_blocks_flac``): returns ``(streams, stats)``,
        one ``bytes`` per stream with the whole FLAC frames this call completed in the engine's FLAC programme — the open frame stays on
        the device until the next call or ``flac_flush()``. Decoded, the samples are ``process_pcm``'s s16 / s24 codes for the same
        render. With listeners attached the render walks ``event_window_blocks()`` windows with the blockwise relay between them; the
        bytes are those of one call. ``drop`` / ``take``: of the frames delivered, the first ``drop`` stay out of the programme and at
        most ``take`` enter it. ``in_fmt``: the inputs are PCM stream arrays in that format (``process_pcm_io``'s), not planar floats.
        ``verify_input`` (``in_fmt`` 'flac'): this call is a programme of its own for option ``flac_in_md5`` — the chunks' decoded samples
        are hashed on the GPU and compared with the MD5 each chunk carries (``FlacChunk.md5``, set by ``FlacReader.read``); the
        statistics carry ``input_md5``, one verdict per input (``verify_end``), and a mismatch raises ``FlacMd5Mismatch`` after the
        render (the frames this call emitted stay in the FLAC programme)."""
        verify = bool(verify_input) and _is_flac(in_fmt)
        if verify:
            self.verify_begin()
        flac = getattr(self._rt, "process_blocks_flac", None)
        if flac is None:
            raise RuntimeError("this engine has no FLAC delivery (process_blocks_flac)")
        if in_fmt is None and len(inputs) != self.num_in:
            raise ValueError(f"Invalid input data; expected {self.num_in} buffers.")
        if int(num_streams) * int(channels_per_stream) != self.num_out:
            raise ValueError(f"Invalid stream layout; expected {self.num_out} channels in all.")
        bs, total = self.block_size, int(num_frames)
        if sample_time is not None:
            self._time = int(sample_time)
        listening = any(self._listeners.values()) and hasattr(self._rt, "event_window_blocks")
        w = max(1, int(self._rt.event_window_blocks())) * bs if listening else max(total, 1)
        inres = getattr(self, "_inres", False) and self.num_in > 0
        flac_in = _is_flac(in_fmt)
        ins = (list(inputs) if flac_in else [np.asarray(a) for a in inputs]) if in_fmt is not None else None
        parts, icur = [], 0
        drop_left, take_left = int(drop), None if take is None else int(take)
        for k in range(0, max(total, 1), w):
            m = min(w, total - k)
            x = None
            if ins is not None:
                ni = self._rt.input_resample_frames(m) if inres else m
                x = []
                for a in ins:
                    if flac_in:
                        x.append(a.at(icur, ni))
                        continue
                    seg = a[icur:icur + ni]
                    if seg.shape[0] < ni:
                        seg = np.concatenate([seg, np.zeros((ni - seg.shape[0],) + a.shape[1:], dtype=a.dtype)])
                    x.append(seg)
                icur += ni
            elif self.num_in:
                x, icur = self._pull(inputs, icur, m)
            nd = self._rt.resample_frames(m)
            d = min(drop_left, nd)
            t = nd - d if take_left is None else min(take_left, nd - d)
            drop_left -= d
            if take_left is not None:
                take_left -= t
            parts.append(flac(x, num_streams, channels_per_stream, m, bits, dither_seed=dither_seed, sample_time=self._time, drop=d, take=t, in_fmt=in_fmt))
            self._time += ((m + bs - 1) // bs) * bs
            events = self._rt.process_queued_events(blockwise=True) if listening else self._rt.process_queued_events()
            for kind, payload in events:
                for cb in self._listeners.get(kind, []):
                    cb(payload)
        if len(parts) == 1:
            streams, stats = parts[0]
        else:
            streams = [b"".join(p[0][s] for p in parts) for s in range(int(num_streams))]
            stats = {"peak": np.max([p[1]["peak"] for p in parts], axis=0), "over": np.sum([p[1]["over"] for p in parts], axis=0, dtype=np.uint64),
                     "nonfinite": np.sum([p[1]["nonfinite"] for p in parts], axis=0, dtype=np.uint64)}
        if verify:
            stats = dict(stats, input_md5=self.verify_end([getattr(a, "md5", None) for a in ins]))
        return streams, stats

    def flac_flush(self):
        """The open remainder of the FLAC programme as one final short frame per stream; the programme is closed until ``flac_reset()``."""
        return self._rt.flac_flush()

    def flac_reset(self) -> None:
        """A new FLAC programme: nothing open, frame number 0."""
        self._rt.flac_reset()

    def flac(self) -> Dict[str, Any]:
        """The FLAC programme so far (``Runtime.flac_read``): per stream the frames emitted, their byte lengths and the STREAMINFO fields."""
        return self._rt.flac_read()

    def _stream_paths(self, path, S: int):
        if isinstance(path, (list, tuple)):
            paths = [str(p) for p in path]
        elif S == 1:
            paths = [str(path)]
        else:
            if "{}" not in str(path):
                raise ValueError("several streams need a list of paths or a path with {} for the stream number")
            paths = [str(path).format(s) for s in range(S)]
        if len(paths) != S:
            raise ValueError(f"{S} streams need {S} paths")
        return paths

    def _flac_files(self, paths, pull, total: int, skip: int, keep: int, bits: int, S: int, G: int, dither_seed, chunk: int, in_fmt=None):
        """``total`` frames rendered in chunks into one FLAC file per stream: a new FLAC programme that leaves the first ``skip``
        delivered frames out and holds ``keep`` (frames cannot be cut on the host: the engine leaves them out in front of the
        encoder), flushed at the end; STREAMINFO patched from ``flac_read`` — with the streams' MD5 where the engine carries option
        ``flac_md5``. ``pull(m)``: the inputs of the next ``m`` engine frames."""
        from .flac import FlacWriter
        self._rt.flac_reset()
        frame = int(self._rt.flac_read()["flac_frame"])
        writers = [FlacWriter(p, bits, G, self.output_sample_rate, frame) for p in paths]
        stats = None
        try:
            for k in range(0, total, chunk):
                m = min(chunk, total - k)
                nd = self._rt.resample_frames(m)
                drop = min(skip, nd)
                take = min(keep, nd - drop)
                skip -= drop
                keep -= take
                streams, st = self.process_flac(pull(m), S, G, m, bits, dither_seed=dither_seed, drop=drop, take=take, in_fmt=in_fmt)
                for wtr, data in zip(writers, streams):
                    wtr.write(data)
                stats = st if stats is None else {"peak": np.maximum(stats["peak"], st["peak"]), "over": stats["over"] + st["over"],
                                                  "nonfinite": stats["nonfinite"] + st["nonfinite"]}
            for wtr, data in zip(writers, self._rt.flac_flush()):
                wtr.write(data)
            got = self._rt.flac_read()
            for s, wtr in enumerate(writers):
                wtr.patch(got["stream_frames"][s], got["min_frame_bytes"][s], got["max_frame_bytes"][s], got["total_samples"][s],
                          md5=got["md5"][s] if got["md5_state"] == 2 else None)
        finally:
            for wtr in writers:
                wtr.close()
        return self._with_loudness(stats)

    def write_flac(self, path, inputs: Sequence[np.ndarray], num_frames: int, bits: int = 16, channels_per_stream: Optional[int] = None,
                   dither_seed: Optional[int] = None, chunk_frames: int = 1 << 20):
        """``write_wav`` into FLAC files (16 or 24 ``bits``), encoded on the GPU: one file per stream of ``channels_per_stream`` channels
        (1 .. 8; default all output channels in one file), block size = option ``flac_frame``. The samples a decoder gets back are
        those of ``write_wav`` in 's16' / 's24' with the same ``dither_seed``. The STREAMINFO MD5 is computed on the GPU where the engine factory sets
        option ``flac_md5`` = 1; without it the field is all zero ("not computed"). Returns the statistics as ``write_wav`` does, over the frames in the files."""
        G = self.num_out if channels_per_stream is None else int(channels_per_stream)
        S = self.num_out // max(G, 1)
        paths = self._stream_paths(path, S)
        bs = self.block_size
        total, skip, keep = self._file_span(num_frames)
        self._qc_window(skip, keep)
        chunk = max(bs, (int(chunk_frames) // bs) * bs)
        cursor = [0]

        def pull(m):
            ni = self._rt.input_resample_frames(m) if getattr(self, "_inres", False) and self.num_in else m
            x = [np.asarray(b)[cursor[0]:cursor[0] + ni] for b in inputs]
            cursor[0] += ni
            return x
        return self._flac_files(paths, pull, total, skip, keep, int(bits), S, G, dither_seed, chunk)

    def loudness(self, weights=None, programmes=None):
        """What the loudness meter (``initialize(loudness_meter=True)``) has measured since the renderer was made or
        ``loudness_reset()``: ``{'integrated_lufs', 'momentary_max_lufs', 'short_term_max_lufs',
        'true_peak_dbtp', 'frames', 'sub_blocks'}`` (EBU R 128 gating; ``-inf`` where nothing passes the gates; the true peak is the
        largest of the programme's channels). ``weights``: one per output channel (default 1.0). ``programmes``: a list of lists of
        channel indices, each metered as a programme of its own (a list of results comes back); default one programme of all channels."""
        from . import loudness as ld
        if not self._loudness:
            raise RuntimeError("the loudness meter is off: initialize(loudness_meter=True)")
        got = self._rt.loudness_read()
        w = np.ones(got["channels"], dtype=np.float64) if weights is None else np.asarray(weights, dtype=np.float64)

        def one(chs):
            chs = [int(c) for c in chs]
            g = ld.gate(got["mean_squares"][chs], w[chs])
            return {"integrated_lufs": g["integrated"], "momentary_max_lufs": g["momentary_max"], "short_term_max_lufs": g["short_term_max"],
                    "true_peak_dbtp": ld.dbtp(max([float(got["true_peak"][c]) for c in chs], default=0.0)),
                    "frames": got["frames"], "sub_blocks": got["sub_blocks"]}
        if programmes is None:
            return one(range(got["channels"]))
        return [one(chs) for chs in programmes]

    def resample(self) -> Dict[str, int]:
        """The converter's plan and clock (``initialize(output_sample_rate=...)``): ``{'up', 'down', 'taps', 'latency_frames',
        'frames_in', 'frames_out'}``."""
        if not self._resample:
            raise RuntimeError("delivery at another rate is off: initialize(output_sample_rate=...)")
        return self._rt.resample_read()

    def resample_reset(self) -> None:
        """A new programme for the converter: time 0, silence in front of it."""
        self._rt.resample_reset()

    def input_resample(self) -> Dict[str, int]:
        """The input converter's plan and clock (``initialize(input_sample_rate=...)``): ``{'up', 'down', 'taps', 'latency_frames',
        'frames_in', 'frames_out'}`` — the latency and ``frames_out`` in engine frames."""
        if not getattr(self, "_inres", False):
            raise RuntimeError("inputs at another rate are off: initialize(input_sample_rate=...)")
        return self._rt.input_resample_read()

    def input_resample_reset(self) -> None:
        """A new programme for the input converter: time 0, silence in front of it."""
        self._rt.input_resample_reset()

    def limiter(self) -> Dict[str, Any]:
        """The limiter's plan and statistics (``initialize(limiter=...)``): ``{'lookahead_frames', 'latency_frames', 'release_frames',
        'link', 'groups', 'frames', 'max_reduction', 'limited_frames'}`` — the last two one per linked group — and
        ``'max_reduction_db'``, the deepest gain reduction of any group in dB (0.0: never limited)."""
        if not getattr(self, "_limiter", False):
            raise RuntimeError("the limiter is off: initialize(limiter=...)")
        got = self._rt.limiter_read()
        worst = float(np.max(got["max_reduction"], initial=0.0))
        got["max_reduction_db"] = 0.0 if worst <= 0.0 else float("inf") if worst >= 1.0 else -20.0 * float(np.log10(1.0 - worst))
        return got

    def limiter_reset(self) -> None:
        """A new programme for the limiter: frame 0, silence in front of it, statistics zero."""
        self._rt.limiter_reset()

    def _file_span(self, num_frames: int, input_frames: bool = False):
        """A file of a converted and / or limited render: (frames to render, delivered frames to drop in front, frames the file
        holds). The converter's latency Do and the limiter's D + 6, both in delivered frames, are taken out together, so frame n of
        the file is the (limited) render at time n * down / up: ceil((Do + D + 6) down / up) further frames are rendered, the first
        Do + D + 6 delivered frames dropped, ceil(num_frames up / down) kept. New programmes start.
        With ``initialize(input_sample_rate=...)`` the input converter's latency Di (engine frames) is taken out with the others: in
        delivered frames it is Di up / down, rounded to nearest where that is not integral — the file then sits less than half a
        delivered frame off. ``input_frames``: ``num_frames`` counts frames of an input file, which render ceil(F L / M) engine
        frames (L / M = engine rate / input rate)."""
        limiting = getattr(self, "_limiter", False)
        if getattr(self, "_noise_shape", False):
            self._rt.noise_shape_reset()        # (a file is a programme of its own for the error feedback too)
        if getattr(self, "_inres", False):
            self._rt.input_resample_reset()
            iinfo = self._rt.input_resample_read()
            n = -((-int(num_frames) * iinfo["up"]) // iinfo["down"]) if input_frames else int(num_frames)
            up, down, lat = 1, 1, 0
            if self._resample:
                self._rt.resample_reset()
                info = self._rt.resample_read()
                up, down, lat = info["up"], info["down"], info["latency_frames"]
            if limiting:
                self._rt.limiter_reset()
                lat += self._rt.limiter_read()["latency_frames"]
            lat += (2 * iinfo["latency_frames"] * up + down) // (2 * down)
            return n + -((-lat * down) // up), lat, -((-n * up) // down)
        if not self._resample and not limiting:
            return int(num_frames), 0, int(num_frames)
        up, down, lat = 1, 1, 0
        if self._resample:
            self._rt.resample_reset()
            info = self._rt.resample_read()
            up, down, lat = info["up"], info["down"], info["latency_frames"]
        if limiting:
            self._rt.limiter_reset()
            lat += self._rt.limiter_read()["latency_frames"]
        return int(num_frames) + -((-lat * down) // up), lat, -((-int(num_frames) * up) // down)

    def noise_shape(self) -> Dict[str, Any]:
        """The noise shaping's coefficients and counts (``initialize(noise_shape=...)``): ``Runtime.noise_shape_read()``."""
        if not getattr(self, "_noise_shape", False):
            raise RuntimeError("noise shaping is off: initialize(noise_shape=...)")
        return self._rt.noise_shape_read()

    def noise_shape_reset(self) -> None:
        """A new programme for the noise shaping: errors zero, counts zero."""
        self._rt.noise_shape_reset()

    def spectrogram(self, flush: bool = False) -> Dict[str, Any]:
        """What the spectrum analyser (``initialize(spectrum={...})``) has emitted since the renderer was made or
        ``spectrogram_reset()``: ``{'frames': float32 [channels, n, columns], 'sums': float64 [channels, columns] (the running sums:
        divided by ``frames_total`` the long-term average spectrum), 'frames_total', 'delivered', 'hop', 'size', ...}`` —
        ``Runtime.spectrum_read`` with the frames of earlier reads in front. ``flush``: the programme is padded with zeros and ended
        first, so the frames that reach beyond its end are included; the next render then starts a new programme and a new
        spectrogram. Powers are linear; ``elementary_amd.spectrum.to_db`` takes the logarithm."""
        if not getattr(self, "_spectrum", False):
            raise RuntimeError("the spectrum analyser is off: initialize(spectrum={...})")
        if flush:
            self._rt.spectrum_flush()
        got = self._rt.spectrum_read()
        if got["first_frame"] == 0:
            self._spectrum_parts = []          # (a new programme began since the last read)
        self._spectrum_parts.append(got["frames"])
        got["frames"] = np.concatenate(self._spectrum_parts, axis=1) if len(self._spectrum_parts) > 1 else got["frames"]
        got["first_frame"] = 0
        self._spectrum_parts = [] if flush else [got["frames"]]
        return got

    def spectrogram_reset(self) -> None:
        """A new programme for the spectrum analyser; what it had emitted is dropped."""
        self._rt.spectrum_reset()
        self._spectrum_parts = []

    def loudness_reset(self) -> None:
        """A new programme for the loudness meter: time 0, zero filter state, no peaks."""
        self._rt.loudness_reset()

    def qc(self) -> Dict[str, Any]:
        """What the inspector (``initialize(qc={...})``) has found since the renderer was made, ``qc_reset()`` or the last file wrapper
        began: ``Runtime.qc_read`` with ``overview`` holding every complete bucket of the programme so far (the buckets of earlier reads
        in front). ``elementary_amd.qc.report`` and ``findings`` derive the figures and the verdicts."""
        if getattr(self, "_qc", None) is None:
            raise RuntimeError("the inspector is off: initialize(qc={...})")
        got = self._rt.qc_read()
        if got["first_bucket"] == 0:
            self._qc_overview = []             # (a new programme began since the last read)
        self._qc_overview.append(got["overview"])
        if len(self._qc_overview) > 1 and all(p.shape[0] == got["overview"].shape[0] for p in self._qc_overview):
            got["overview"] = np.concatenate(self._qc_overview, axis=1)
        self._qc_overview = [got["overview"]]
        got["first_bucket"] = 0
        return got

    def qc_reset(self) -> None:
        """A new programme for the inspector; what it had found is dropped."""
        if getattr(self, "_qc", None) is None:
            raise RuntimeError("the inspector is off: initialize(qc={...})")
        self._rt.qc_reset()
        self._qc_overview = []

    def _qc_window(self, skip: int, keep: int) -> None:
        """A file wrapper begins: a new programme whose window is the frames the file holds, not the latencies in front of them."""
        if getattr(self, "_qc", None) is not None and keep > 0:
            self._rt.qc(dict(self._qc, skip=int(skip), limit=int(keep)))
            self._qc_overview = []

    def _with_loudness(self, stats):
        if self._loudness and stats is not None:
            got = self.loudness()
            stats = dict(stats, integrated_lufs=got["integrated_lufs"], true_peak_dbtp=got["true_peak_dbtp"])
        if getattr(self, "_limiter", False) and stats is not None:
            stats = dict(stats, limiter_max_reduction_db=self.limiter()["max_reduction_db"])
        if getattr(self, "_qc", None) is not None and stats is not None:
            stats = dict(stats, qc=self.qc())
        return stats

    def write_wav(self, path, inputs: Sequence[np.ndarray], num_frames: int, fmt="s16", channels_per_stream: Optional[int] = None,
                  dither_seed: Optional[int] = None, chunk_frames: int = 1 << 20):
        """Render ``num_frames`` frames into RIFF/WAVE files, ``chunk_frames`` (rounded to whole blocks) per engine call: one file per
        stream of ``channels_per_stream`` channels (default: all output channels in one file). ``path``: the file's name, or — for
        more than one stream — a list of names or a name with ``{}`` for the stream number. Returns the statistics of the render; with the loudness
        meter on they carry ``integrated_lufs`` and ``true_peak_dbtp`` as well — ``loudness()`` of the meter's programme so far (call
        ``loudness_reset()`` first for figures of this file alone); with the limiter on, ``limiter_max_reduction_db`` of this file."""
        from .wav import WavWriter
        G = self.num_out if channels_per_stream is None else int(channels_per_stream)
        S = self.num_out // max(G, 1)
        if isinstance(path, (list, tuple)):
            paths = list(path)
        elif S == 1:
            paths = [str(path)]
        else:
            if "{}" not in str(path):
                raise ValueError("several streams need a list of paths or a path with {} for the stream number")
            paths = [str(path).format(s) for s in range(S)]
        if len(paths) != S:
            raise ValueError(f"{S} streams need {S} paths")
        bs = self.block_size
        total, skip, keep = self._file_span(num_frames)
        self._qc_window(skip, keep)
        chunk = max(bs, (int(chunk_frames) // bs) * bs)
        writers = [WavWriter(p, fmt if isinstance(fmt, str) else {1: "s16", 2: "s24", 3: "f32"}[int(fmt)], G, self.output_sample_rate) for p in paths]
        stats = None
        try:
            icur = 0                          # input frames consumed so far (initialize(input_sample_rate=...): not the engine's count)
            for k in range(0, total, chunk):
                m = min(chunk, total - k)
                ni = self._rt.input_resample_frames(m) if getattr(self, "_inres", False) and self.num_in else m
                streams, st, _ = self.process_pcm([np.asarray(b)[icur:icur + ni] for b in inputs], S, G, m, fmt, dither_seed=dither_seed)
                icur += ni
                drop = min(skip, len(streams[0])) if streams else 0
                take = min(keep, (len(streams[0]) if streams else 0) - drop)
                skip -= drop
                keep -= take
                for wtr, a in zip(writers, streams):
                    wtr.write(a[drop:drop + take])
                if stats is None:
                    stats = st
                else:
                    stats = {"peak": np.maximum(stats["peak"], st["peak"]), "over": stats["over"] + st["over"], "nonfinite": stats["nonfinite"] + st["nonfinite"]}
        finally:
            for wtr in writers:
                wtr.close()
        return self._with_loudness(stats)

    def process_pcm_io(self, in_streams: Sequence[np.ndarray], in_fmt, num_frames: Optional[int] = None, out_fmt=None,
                       num_streams: Optional[int] = None, channels_per_stream: Optional[int] = None, dither_seed: Optional[int] = None,
                       want_float: bool = False, sample_time: Optional[int] = None, verify_input: bool = False):
        """``process`` / ``process_pcm`` fed with interleaved PCM that is unpacked on the GPU (``Runtime.process_blocks_pcm_io``):
        ``in_streams`` are arrays in stream layout (``WavReader.read``, or what ``process_pcm`` returns) that together hold the
        ``num_input_channels`` input channels; a stream shorter than ``num_frames`` is padded with silence. ``in_fmt`` 'flac': the
        streams are ``FlacChunk`` objects (``FlacReader.read``) — FLAC frames that are decoded on the GPU. ``out_fmt`` None: returns
        float32 ``[num_output_channels, num_frames]``; else ``(streams, stats, planar)`` as ``process_pcm`` does. With listeners attached
        the render walks ``event_window_blocks()`` windows with the blockwise relay between them, as ``process`` does. With
        ``initialize(limiter=...)`` what comes back is limited and carries the limiter's latency: frame n is the limited render at
        n - latency_frames. ``verify_input`` (``in_fmt`` 'flac'): this call is a programme of its own for option ``flac_in_md5`` — the
        chunks' decoded samples are hashed on the GPU and compared with the MD5 each chunk carries (``FlacChunk.md5``, set by
        ``FlacReader.read``); the verdicts (``verify_end``) are ``self.input_md5`` and, where statistics come back, their
        ``input_md5``; a mismatch raises ``FlacMd5Mismatch`` after the render."""
        verify = bool(verify_input) and _is_flac(in_fmt)
        if verify:
            self.verify_begin()
        pcm_io = getattr(self._rt, "process_blocks_pcm_io", None)
        if pcm_io is None:
            raise RuntimeError("this engine takes no PCM input (process_blocks_pcm_io)")
        flac_in = _is_flac(in_fmt)        # ``in_streams``: FlacChunk objects (``FlacReader.read``), decoded on the GPU
        ins = list(in_streams) if flac_in else [np.asarray(a) for a in in_streams]
        if sum(int(a.channels if flac_in else a.shape[1]) for a in ins) != self.num_in:
            raise ValueError(f"Invalid input data; expected {self.num_in} channels in all.")
        if out_fmt is not None and int(num_streams) * int(channels_per_stream) != self.num_out:
            raise ValueError(f"Invalid stream layout; expected {self.num_out} channels in all.")
        bs = self.block_size
        inres = getattr(self, "_inres", False) and bool(ins)
        total = int(num_frames) if num_frames is not None else (int(ins[0].count if flac_in else ins[0].shape[0]) if ins else 0)
        if inres and num_frames is None:          # (the streams' length in ENGINE frames)
            iinfo = self._rt.input_resample_read()
            total = -((-total * iinfo["up"]) // iinfo["down"])
        if sample_time is not None:
            self._time = int(sample_time)
        listening = any(self._listeners.values()) and hasattr(self._rt, "event_window_blocks")
        w = max(1, int(self._rt.event_window_blocks())) * bs if listening else max(total, 1)
        parts = []
        icur = 0                                  # input frames consumed so far
        for k in range(0, max(total, 1), w):
            m = min(w, total - k)
            ni = self._rt.input_resample_frames(m) if inres else m
            x = []
            for a in ins:
                if flac_in:               # (the engine looks the covering frames up; past the stream's end is silence)
                    x.append(a.at(icur, ni))
                    continue
                seg = a[icur:icur + ni]
                if seg.shape[0] < ni:     # (silence is all-zero bytes in every format)
                    seg = np.concatenate([seg, np.zeros((ni - seg.shape[0],) + a.shape[1:], dtype=a.dtype)])
                x.append(seg)
            icur += ni
            parts.append(pcm_io(x, in_fmt, self.num_out, m, out_fmt, num_streams, channels_per_stream, dither_seed=dither_seed,
                                want_float=want_float, sample_time=self._time))
            self._time += ((m + bs - 1) // bs) * bs
            events = self._rt.process_queued_events(blockwise=True) if listening else self._rt.process_queued_events()
            for kind, payload in events:
                for cb in self._listeners.get(kind, []):
                    cb(payload)
        verdicts = self.verify_end([getattr(a, "md5", None) for a in ins]) if verify else None
        if out_fmt is None:
            return parts[0] if len(parts) == 1 else np.concatenate(parts, axis=1)
        if len(parts) == 1:
            streams, stats, planar = parts[0]
        else:
            streams = [np.concatenate([p[0][s] for p in parts]) for s in range(int(num_streams))]
            stats = {"peak": np.max([p[1]["peak"] for p in parts], axis=0), "over": np.sum([p[1]["over"] for p in parts], axis=0, dtype=np.uint64),
                     "nonfinite": np.sum([p[1]["nonfinite"] for p in parts], axis=0, dtype=np.uint64)}
            planar = np.concatenate([p[2] for p in parts], axis=1) if want_float else None
        if verify:
            stats = dict(stats, input_md5=verdicts)
        return streams, stats, planar

    def process_wav(self, in_paths, out_paths, out_fmt="s16", channels_per_stream: Optional[int] = None, num_frames: Optional[int] = None,
                    dither_seed: Optional[int] = None, chunk_frames: int = 1 << 20, verify_input: bool = False):
        """RIFF/WAVE files through the graph into RIFF/WAVE files, ``chunk_frames`` (rounded to whole blocks) per engine call; the samples
        cross the host as they lie in the files and are converted on the GPU in both directions (``out_fmt`` 'flac16' / 'flac24': FLAC
        files instead, encoded on the GPU — ``write_flac``'s). An input that starts with ``fLaC`` is read by ``FlacReader``: its frames
        cross the host compressed and are decoded on the GPU; with ``verify_input`` the decoded samples' MD5 is computed there too (option
        ``flac_in_md5``: no sample reaches the host for it) and compared with what each file's STREAMINFO announces — the statistics
        then carry ``input_md5``, one of 'ok' / 'absent' / 'incomplete' / 'mismatch' per input file (``verify_end``), and a mismatch
        raises ``FlacMd5Mismatch`` AFTER the output files have been closed: they are left in place and named in the exception,
        deleting them is the caller's decision. ``in_paths``: one name or a list —
        the files' channels become the input channels in file order (files of one format, one channel count and the renderer's
        sample rate — or, with ``initialize(input_sample_rate=...)``, that rate: a file of F frames then renders ceil(F L / M) engine
        frames, L / M = engine rate / input rate, and the input converter's latency is taken out with the others, to under half a
        delivered frame). ``out_paths`` / ``channels_per_stream``: as ``write_wav``'s ``path``. ``num_frames``: frames to render, default
        the (longest) input's length; longer than that — a reverb's tail — renders the rest from silence. Returns the statistics
        (with the loudness meter on: ``integrated_lufs`` and ``true_peak_dbtp`` of the meter's programme so far included, as ``write_wav``;
        with the limiter on: ``limiter_max_reduction_db`` of this file)."""
        from .flac import FlacReader
        from .wav import WavReader, WavWriter
        ins = [str(in_paths)] if isinstance(in_paths, (str, bytes)) or hasattr(in_paths, "__fspath__") else [str(p) for p in in_paths]
        G = self.num_out if channels_per_stream is None else int(channels_per_stream)
        S = self.num_out // max(G, 1)
        if isinstance(out_paths, (list, tuple)):
            outs = [str(p) for p in out_paths]
        elif S == 1:
            outs = [str(out_paths)]
        else:
            if "{}" not in str(out_paths):
                raise ValueError("several streams need a list of paths or a path with {} for the stream number")
            outs = [str(out_paths).format(s) for s in range(S)]
        if len(outs) != S:
            raise ValueError(f"{S} streams need {S} paths")
        fmt = out_fmt if isinstance(out_fmt, str) else {1: "s16", 2: "s24", 3: "f32"}[int(out_fmt)]
        flac_bits = {"flac16": 16, "flac24": 24}.get(fmt.lower())
        readers, writers, stats = [], [], None
        try:
            for p in ins:
                with open(p, "rb") as probe:
                    is_flac = probe.read(4) == b"fLaC"
                readers.append(FlacReader(p) if is_flac else WavReader(p))      # (a FLAC file is decoded on the GPU: its frames cross the host as they are)
            for r in readers:
                if r.sample_rate != int(round(getattr(self, "input_sample_rate", self.sample_rate))):
                    raise ValueError(f"sample rate {r.sample_rate} of an input file, the renderer runs at {int(round(self.sample_rate))}")
                if (r.fmt, r.channels) != (readers[0].fmt, readers[0].channels):
                    raise ValueError(f"input files of one kind are expected: {readers[0].fmt} x {readers[0].channels} and {r.fmt} x {r.channels}")
            if sum(r.channels for r in readers) != self.num_in:
                raise ValueError(f"Invalid input data; expected {self.num_in} channels in all.")
            bs = self.block_size
            inres = getattr(self, "_inres", False) and bool(readers)
            if num_frames is not None or not inres:
                total, skip, keep = self._file_span(int(num_frames) if num_frames is not None else max([r.frames for r in readers], default=0))
            else:
                total, skip, keep = self._file_span(max(r.frames for r in readers), input_frames=True)
            self._qc_window(skip, keep)
            chunk = max(bs, (int(chunk_frames) // bs) * bs)
            in_fmt = readers[0].fmt if readers else "s16"
            verify = bool(verify_input) and bool(readers) and _is_flac(in_fmt)
            if verify:
                self.verify_begin()
            if flac_bits is not None:         # FLAC files: encoded on the GPU, the latencies left out in front of the encoder
                def pull(m):
                    return [r.read(self._rt.input_resample_frames(m) if inres else m) for r in readers]
                stats = self._flac_files(outs, pull, total, skip, keep, flac_bits, S, G, dither_seed, chunk, in_fmt=in_fmt if readers else None)
                total = 0                     # (rendered)
            else:
                writers = [WavWriter(p, fmt, G, self.output_sample_rate) for p in outs]
            for k in range(0, total, chunk):
                m = min(chunk, total - k)
                ni = self._rt.input_resample_frames(m) if inres else m
                streams, st, _ = self.process_pcm_io([r.read(ni) for r in readers], in_fmt, m, fmt, S, G, dither_seed=dither_seed)
                drop = min(skip, len(streams[0])) if streams else 0
                take = min(keep, (len(streams[0]) if streams else 0) - drop)
                skip -= drop
                keep -= take
                for wtr, a in zip(writers, streams):
                    wtr.write(a[drop:drop + take])
                if stats is None:
                    stats = st
                else:
                    stats = {"peak": np.maximum(stats["peak"], st["peak"]), "over": stats["over"] + st["over"], "nonfinite": stats["nonfinite"] + st["nonfinite"]}
        finally:
            expected = [getattr(r, "md5", None) for r in readers]
            for x in readers + writers:
                x.close()
        if flac_bits is None:
            stats = self._with_loudness(stats)
        if verify:          # (the outputs are closed: a mismatch leaves them in place and names them)
            stats = dict(stats or {}, input_md5=self.verify_end(expected, output=outs))
        return stats

    def update_virtual_file_system(self, vfs: Dict[str, np.ndarray]) -> None:
        for k, v in vfs.items():
            self._rt.add_shared_resource(k, v)

    def update_virtual_file_system_files(self, files: Dict[str, str], resample: bool = True, verify: bool = False) -> Dict[str, bool]:
        """Shared resources straight from audio files, decoded on the GPU (``Runtime.add_shared_resource_pcm``): ``{name: path}``. A
        file that starts with ``fLaC`` is read by ``FlacReader`` (its compressed frames cross the host link), anything else by
        ``WavReader`` (s16 / s24 / f32). A file whose rate is not the engine's is converted with the centred filter, so it plays at its
        own pitch and length; ``resample=False`` takes its samples as they are, as ``update_virtual_file_system`` does with floats.
        Returns ``{name: inserted}`` (False: the name was taken). ``verify``: the samples decoded from a FLAC file are hashed on the GPU
        during the load (option ``flac_in_md5``) and the digest — of the FILE's samples, also where the resource is converted — is
        compared with what its STREAMINFO announces; ``self.resource_md5[name]`` is 'ok' / 'absent' / 'incomplete' / 'mismatch', and a
        mismatch raises ``FlacMd5Mismatch`` (``.stream``: the name) once that file is loaded. The resource STAYS under its name
        (resources are insert-only): pruning it, or never using it, is the caller's decision."""
        from .flac import FlacReader
        from .runtime import FlacMd5Mismatch, flac_md5_verdict
        from .wav import WavReader
        done = {}
        if verify:
            self._rt.set_option("flac_in_md5", 1)
            self.resource_md5 = getattr(self, "resource_md5", {})
        for name, path in files.items():
            with open(path, "rb") as f:
                is_flac = f.read(4) == b"fLaC"
            reader = FlacReader(path) if is_flac else WavReader(path)
            try:
                rate = reader.sample_rate if resample else None
                data = reader.read(reader.frames)
                done[name] = self._rt.add_shared_resource_pcm(name, data, None if is_flac else reader.fmt, reader.channels, rate)
                if verify and is_flac and done[name]:
                    got = self._rt.shared_resource_md5(name)
                    self.resource_md5[name] = flac_md5_verdict(got["state"], got["md5"], reader.md5)
                    if self.resource_md5[name] == "mismatch":
                        raise FlacMd5Mismatch(name, reader.md5, got["md5"])
            finally:
                reader.close()
        return done

    def prune_virtual_file_system(self) -> None:
        self._rt.prune_shared_resources()

    def reset(self) -> None:
        self._rt.reset()

    def gc(self) -> List[int]:
        return self._rt.gc()

    def set_current_time(self, t: int) -> None:
        self._time = int(t)

    def set_current_time_ms(self, ms: float) -> None:
        self._time = int(ms * 0.001 * self.sample_rate)
