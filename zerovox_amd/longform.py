"""Long-form synthesis: a paragraph is split into sentences, the sentences are synthesised in batches into one device buffer, and the
rows are trimmed, faded and joined -- with the pauses the punctuation asks for -- into ONE waveform on the device (include/zvx.h, zvx_join).
Not in the reference: its entry points take one utterance (synthesize.py:213-239)."""
from __future__ import annotations

import numpy as np

MAX_CHARS = 200                  # BASELINE's workload is 7 frames per phoneme: 200 x 7 = 1400 frames stays under the FS2 decoder's 1750-frame table
PAUSES_MS = {".": 350, ";": 250, ",": 120, " ": 0}     # pause behind a piece, by the class of the character that closed it
_CLOSING = {".": ".", "!": ".", "?": ".", ";": ";", ":": ";"}
TRIM_FRAME, TRIM_HOP = 2048, 512                       # librosa.effects.trim's defaults, as mels.trim_silence
LOUDNESS_MODES = {"paragraph": True, "sentence": False}   # -> zvx_normalize's ZVX_LOUD_COMMON / ZVX_LOUD_PER_ROW


def peak_ceiling(peak_db):
    """sample-peak ceiling in dBFS -> the linear ceiling of zvx_loudness_params (None: no ceiling)"""
    return 0.0 if peak_db is None else float(10.0 ** (float(peak_db) / 20.0))


def limit_keywords(limiter, limiter_ms, peak_db):
    """the limiter keywords of tts / tts_long -> Context.limit_device keywords, or None (limiter off)"""
    if not limiter:
        return None
    if peak_db is None:
        raise ValueError("limiter=True needs a ceiling: peak_db is None")
    return dict(ceiling=peak_ceiling(peak_db), window_ms=float(limiter_ms), oversample=4)


def _has_phone(s):
    return any(ch.isalnum() for ch in s)


def _split_long(piece, closing, max_chars):
    """a piece longer than max_chars: cut at the last ',' before the limit, failing that at the last blank, failing that at the limit"""
    out = []
    while len(piece) > max_chars:
        cut, cls = piece.rfind(",", 0, max_chars), ","
        if cut <= 0:
            cut, cls = piece.rfind(" ", 0, max_chars), " "
        if cut <= 0:
            cut, cls = max_chars - 1, " "
        out.append((piece[:cut + 1], cls))
        piece = piece[cut + 1:]
    out.append((piece, closing))
    return out


def split_sentences(text, max_chars=MAX_CHARS):
    """-> [(sentence, closing)] in text order.  The text is cut after '.', '!', '?', ';' or ':' (runs of them stay together) where white
    space or the end follows; a piece longer than max_chars is cut again (_split_long).  closing is the class of what ended the piece:
    "." (. ! ? and the end of the text), ";" (; :), "," or " ".  Pieces without a letter or digit -- nothing to pronounce -- are dropped,
    every other piece is stripped of surrounding white space: "".join of the pieces is the text minus white space (and minus such pieces)."""
    if max_chars < 1:
        raise ValueError("max_chars must be positive")
    pieces, start, i, n = [], 0, 0, len(text)
    while i < n:
        if text[i] in _CLOSING:
            j = i
            while j + 1 < n and text[j + 1] in _CLOSING:
                j += 1
            if j + 1 == n or text[j + 1].isspace():
                pieces.append((text[start:j + 1], _CLOSING[text[j]]))
                start = j + 1
            i = j + 1
        else:
            i += 1
    if start < n:
        pieces.append((text[start:], "."))
    out = []
    for piece, closing in pieces:
        for sub, cls in _split_long(piece.strip(), closing, max_chars):
            sub = sub.strip()
            if sub and _has_phone(sub):
                out.append((sub, cls))
    return out


def synthesize_long(tts, text, spkemb, *, pauses=None, trim_db=40.0, keep_ms=20, fade_ms=5, max_batch=32, max_frames=2048, pcm16=False,
                    durations=None, max_chars=MAX_CHARS, prosody=None, loudness=None, peak_db=-1.0, loudness_mode="paragraph",
                    limiter=False, limiter_ms=5.0, denoise=None, report=False, watermark=None, eq=None):
    """The body of ZeroVoxTTS.tts_long (see there).  prosody: Prosody.create keywords applied to every sentence, or None.  denoise: None or
    Context.denoise_device keywords (strength, floor).  watermark: None or watermark.params(...) (key and the embedder's parameters).
    eq: None or equaliser.params(...) (taps, delay)."""
    from . import _lib
    if loudness_mode not in LOUDNESS_MODES:
        raise ValueError(f"loudness_mode: {loudness_mode!r} is none of {sorted(LOUDNESS_MODES)}")
    lim = limit_keywords(limiter, limiter_ms, peak_db)
    ctx = tts.model.ctx
    native = ctx.get_int("sampling_rate")
    out_rate = ctx.get_int("out_rate") or native
    hop = ctx.hop
    items = []
    for sentence, closing in split_sentences(text, max_chars):
        ph, pu = tts.text2phonemeids(sentence)
        if ph:
            items.append((sentence, closing, ph, pu))
    if not items:
        return np.array([[0.0]], dtype=np.float32), []          # the reference's sentinel waveform (synthesize.py:213-239)
    N = len(items)
    if durations is not None and len(durations) != N:
        raise ValueError(f"durations: {len(durations)} lists for {N} sentences")
    ms = dict(PAUSES_MS)
    ms.update(pauses or {})
    gaps = [int(round(ms[c] * native / 1000.0)) for _, c, _, _ in items]
    gaps[-1] = 0
    max_batch = max(1, int(max_batch))
    stride = int(max_frames) * hop                               # samples per row of the device buffer: a longer sentence is ZVX_E_BUFFER
    spk = np.asarray(spkemb, np.float32).reshape(1, -1)
    mel_len = np.zeros(N, np.int32)
    durs = []
    bias = tts.model.denoise_bias if denoise is not None else None      # (first use runs the vocoder: before anything is queued)
    buf = ctx.dev_alloc(N * stride * 4)
    try:
        for b0 in range(0, N, max_batch):
            grp = items[b0:b0 + max_batch]
            B, Tmax = len(grp), max(len(it[2]) for it in grp)
            phoneme, puncts = np.zeros((B, Tmax), np.int32), np.zeros((B, Tmax), np.int32)
            T = np.array([len(it[2]) for it in grp], np.int32)
            dur = None if durations is None else np.zeros((B, Tmax), np.int32)
            for i, it in enumerate(grp):
                phoneme[i, :T[i]], puncts[i, :T[i]] = it[2], it[3]
                if dur is not None:
                    d = np.asarray(durations[b0 + i], np.int32)
                    if d.shape != (T[i],):
                        raise ValueError(f"durations[{b0 + i}]: {d.shape[0] if d.ndim == 1 else d.shape} entries for {T[i]} phonemes")
                    dur[i, :T[i]] = d
            r = ctx.synthesize(phoneme, puncts, T, np.repeat(spk, B, axis=0), dur, np.full(B, 689, np.int32), want_mel=False,
                               Lmax_cap=int(max_frames), wav_device_ptr=buf + b0 * stride * 4, wav_stride=stride, no_sync=True,
                               native_rate=True, prosody=prosody)
            mel_len[b0:b0 + B] = r["mel_len"]
            if int(r["mel_len"].min()) < 2:
                raise ValueError(f"predicted mel length {int(r['mel_len'].min())} is too short to synthesise")
            d = ctx.fetch("duration", (B, Tmax)).astype(np.int32)
            durs += [d[i, :T[i]].copy() for i in range(B)]
        frame, hp = TRIM_FRAME, TRIM_HOP
        keep, fade = int(round(keep_ms * native / 1000.0)), int(round(fade_ms * native / 1000.0))
        kw = dict(frame=frame, hop=hp, top_db=float(trim_db), keep=keep, fade=fade)
        lengths = mel_len.astype(np.int64) * hop
        lufs, gain = [None] * N, [None] * N
        # every step is ONE call over all rows, in place, behind the queued synthesis calls; under a limiter the gain has no peak ceiling
        loud, limited = tts.model.post_chain_device(
            buf, lengths, stride, denoise=None if denoise is None else dict(denoise, bias=bias), watermark=watermark,
            loudness=None if loudness is None else dict(target=loudness, peak_ceiling=0.0 if lim else peak_ceiling(peak_db),
                                                        common=LOUDNESS_MODES[loudness_mode]), limiter=lim, rate=native,
            **({} if eq is None else {"eq": eq}))
        if loud is not None:
            lufs, gain = [float(v) for v in loud[0]], [float(v) for v in loud[2]]
        if lim:
            min_gain = limited[1]
        if out_rate == native and report and not pcm16:          # the joined row stays on the device until it is measured
            cap = int(lengths.sum()) + int(sum(gaps))
            joined = ctx.dev_alloc(max(cap, 1) * 4)
            try:
                total, pos, begin, ln = ctx.join_device(buf, lengths, stride, gaps, out_device_ptr=joined, out_capacity=cap, **kw)
                tts.model.loudness_report_device(joined, total, native)
                wav = ctx.dev_to_host(joined, (total,), np.float32) if total else np.zeros(0, np.float32)
            finally:
                ctx.dev_free(joined)
            start = [int(p) for p in pos]
            count = [int(v) for v in ln]
        elif out_rate == native:
            wav, pos, begin, ln = ctx.join_device(buf, lengths, stride, gaps, pcm16=pcm16, **kw)
            start = [int(p) for p in pos]
            count = [int(v) for v in ln]
        else:
            cap = int(lengths.sum()) + int(sum(gaps))
            joined = ctx.dev_alloc(max(cap, 1) * 4)
            try:
                total, pos, begin, ln = ctx.join_device(buf, lengths, stride, gaps, out_device_ptr=joined, out_capacity=cap, **kw)
                wav = ctx.resample_device(joined, total, native, out_rate, pcm16=pcm16)
            finally:
                ctx.dev_free(joined)
            start = [_lib.resampled_len(int(p), native, out_rate) for p in pos]
            count = [_lib.resampled_len(int(p) + int(v), native, out_rate) - s for p, v, s in zip(pos, ln, start)]
    finally:
        try:
            ctx.sync()                                           # queued launches still write the buffer
        finally:
            ctx.dev_free(buf)
    if report and (out_rate != native or pcm16):                 # converted or int16: the waveform is measured as it arrived
        tts.loudness_report(wav, out_rate)
    segments = [dict(text=items[i][0], start=start[i], samples=count[i], mel_len=int(mel_len[i]), trim=int(begin[i]), durations=durs[i])
                for i in range(N)]
    if loudness is not None:
        for i, s in enumerate(segments):
            s["lufs"], s["gain"] = lufs[i], gain[i]
    if lim:
        for i, s in enumerate(segments):
            s["min_gain"] = float(min_gain[i])
    return wav, segments
