"""Speaker enrolment on the device, the parts that need no GPU: header / binding agreement of zvx_spkemb_wav and ZVX_DEVICE_SPK, the tests'
float reference (tests/enroll_ref.py) against the oracle front end on a sliced array, the properties the GPU tests rely on in their
clips, and the grouping of ZeroVoxTTS.speaker_embed_batch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import enroll_ref as E
import join_ref as J
from oracle import mel_oracle as MO
from zerovox_amd import _lib, config as zcfg
from zerovox_amd.synthesize import ZeroVoxTTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = [(2048, 512, 40.0, 0), (2048, 512, 40.0, 441), (1024, 256, 25.0, 1002), (400, 160, 60.0, 3), (2048, 512, 0.0, 0)]


def header_code():
    hdr = open(os.path.join(ROOT, "include", "zvx.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_exports_and_signature_agree_on_zvx_spkemb_wav():
    code = header_code()
    m = re.search(r"zvx_status\s+zvx_spkemb_wav\s*\((.*?)\)\s*;", code, flags=re.S)
    assert m, "zvx_spkemb_wav not declared"
    assert "zvx_spkemb_wav" in _lib.EXPORTS
    want = []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        if "zvx_ref_params*" in arg.replace(" *", "*"):
            want.append(C.POINTER(_lib.RefParams))
        elif "*" in arg:
            want.append(C.c_void_p)
        else:
            assert arg.startswith("int "), arg
            want.append(C.c_int)
    names = [re.findall(r"[A-Za-z_]+", a)[-1] for a in m.group(1).split(",")]
    assert names == ["ctx", "wav", "nsamples", "B", "Nmax", "rate", "params", "out", "begin", "end", "frames", "flags"], names
    lib = _lib.load()
    assert list(lib.zvx_spkemb_wav.argtypes) == want


def test_ref_params_has_the_five_fields_in_header_order():
    m = re.search(r"typedef struct zvx_ref_params \{(.*?)\} zvx_ref_params;", header_code(), flags=re.S)
    assert m, "zvx_ref_params not declared"
    fields = []
    for decl in m.group(1).split(";"):
        toks = decl.replace(",", " ").split()
        if toks:
            fields += [(name, toks[0]) for name in toks[1:]]
    ctype = {"int32_t": C.c_int32, "float": C.c_float}
    assert [n for n, _ in fields] == ["frame", "hop", "top_db", "keep", "max_samples"]
    assert [(n, ctype[t]) for n, t in fields] == list(_lib.RefParams._fields_), fields
    assert C.sizeof(_lib.RefParams) == 20


def test_device_spk_flag_is_64():
    assert re.search(r"\bZVX_DEVICE_SPK\s*=\s*64\b", header_code()) and _lib.ZVX_DEVICE_SPK == 64
    others = (_lib.ZVX_DEVICE_OUT, _lib.ZVX_NO_SYNC, _lib.ZVX_PCM16, _lib.ZVX_DEVICE_IN, _lib.ZVX_HOST_ASYNC, _lib.ZVX_NATIVE_RATE)
    assert all(_lib.ZVX_DEVICE_SPK & f == 0 for f in others)


def test_reference_window_mel_equals_the_oracle_on_the_sliced_array():
    """the index arithmetic of enroll_ref.window_mel (mirror about the window's own ends, inside the row) is get_mel_from_wav of the slice"""
    a = E.audio_args(zcfg.medium_modelcfg("styletts"))
    clips = E.make_clips(0)
    for x, (begin, end) in zip(clips, ((3001, 30002), (0, 7903), (4999, 20011), (1702, 2215), (0, 1501))):
        x = x.copy()
        got = E.window_mel(x, begin, end, **a)
        want, _ = MO.get_mel_from_wav(x[begin:end], a["sampling_rate"], a["fft_size"], a["hop_size"], a["win_length"], a["num_mels"], a["fmin"], a["fmax"])
        assert got.shape == (E.frames_ref(end - begin), a["num_mels"]) and np.array_equal(got, want.T)
        x[:begin] = np.nan; x[end:] = np.nan                                       # nothing outside the window is read
        assert np.array_equal(E.window_mel(x, begin, end, **a), got)


def test_clips_have_what_the_gpu_tests_rely_on():
    """from the reference alone: no frame near the trim threshold, begin and end on every residue mod 4, a row left whole, every window long
    enough for the speaker encoder -- at the model's rate and for the clips given at 16 and 48 kHz"""
    res_b, res_e = set(), set()
    for rate in (E.NATIVE, 16000, 48000):
        rows = [E.at_model_rate(x, rate) for x in E.make_clips(0, rate)]
        assert len(rows) == 5 and 1400 <= len(rows[4]) < 2048 and max(len(r) for r in rows) <= 36000
        for frame, hop, top_db, keep in GRID:
            for b, y in enumerate(rows):
                begin, end, worst = E.window_ref(y, frame, hop, top_db, keep)
                assert worst > 1e3 * J.AMBIGUOUS, (rate, frame, hop, top_db, b, worst)
                assert end - begin >= 512, (rate, frame, hop, top_db, keep, b, begin, end)
                if rate == E.NATIVE:
                    res_b.add(begin % 4); res_e.add(end % 4)
        b4, e4, _ = E.window_ref(rows[4])
        assert (b4, e4) == (0, len(rows[4]))                                       # shorter than the frame: left whole
        trimmed = sum(E.window_ref(y)[:2] != (0, len(y)) for y in rows)
        assert trimmed >= 4, trimmed
    assert res_b == {0, 1, 2, 3} and res_e == {0, 1, 2, 3}, (res_b, res_e)


class StubContext:
    hidden = 6

    def __init__(self):
        self.calls = []

    def spkemb_wav(self, rows, rate=None, **kw):
        self.calls.append((int(rate), [len(r) for r in rows], kw))
        emb = np.zeros((len(rows), self.hidden), np.float32)
        for i, r in enumerate(rows):
            emb[i] = len(r) + np.arange(self.hidden) / 10.0                        # a row is recognised by its length
        z = np.zeros(len(rows), np.int32)
        return emb, z, z, z


def stub_synth():
    s = ZeroVoxTTS.__new__(ZeroVoxTTS)
    s._sampling_rate = 22050
    s._model = type("M", (), {})()
    s._model.ctx = StubContext()
    return s


def test_speaker_embed_batch_groups_by_rate_and_keeps_input_order():
    s = stub_synth()
    lens = [700, 710, 720, 730, 740]
    wavs = [np.zeros(n, np.float32) for n in lens]
    out = s.speaker_embed_batch(wavs, [22050, 16000, 22050, 48000, 16000])
    calls = s._model.ctx.calls
    assert sorted((r, l) for r, l, _ in calls) == [(16000, [710, 740]), (22050, [700, 720]), (48000, [730])]      # one call per distinct rate
    assert all(kw == dict(top_db=40.0, max_samples=0) for _, _, kw in calls)
    assert out.shape == (5, 1, 6) and out.dtype == np.float32
    assert [int(out[i, 0, 0]) for i in range(5)] == lens                           # input order
    s = stub_synth()
    out = s.speaker_embed_batch(wavs, top_db=25.0, max_seconds=1.5)                 # no rate: the model's, one call
    assert s._model.ctx.calls == [(22050, lens, dict(top_db=25.0, max_samples=33075))]
    s = stub_synth()
    s.speaker_embed_batch(wavs[:2], 16000)                                          # a scalar rate
    assert [c[:2] for c in s._model.ctx.calls] == [(16000, [700, 710])]
    with pytest.raises(ValueError):
        s.speaker_embed_batch(wavs, [22050, 16000])


def test_speaker_embed_files_reads_every_file_at_its_own_rate(tmp_path):
    import wave
    s = stub_synth()
    paths = []
    for i, (sr, n) in enumerate(((16000, 800), (22050, 900), (16000, 1000))):
        p = tmp_path / f"ref{i}.wav"
        with wave.open(str(p), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr)
            w.writeframes((np.arange(n) % 100).astype(np.int16).tobytes())
        paths.append(p)
    out = s.speaker_embed_files(paths)
    assert sorted(c[:2] for c in s._model.ctx.calls) == [(16000, [800, 1000]), (22050, [900])]
    assert [int(out[i, 0, 0]) for i in range(3)] == [800, 900, 1000]
