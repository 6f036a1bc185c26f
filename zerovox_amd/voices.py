"""Voice matching: a library of speaker embeddings that lives on the device, searched there (include/zvx.h: zvx_spk_score, zvx_spk_topk),
and the report of whose voice a waveform carries (ZeroVoxTTS.voice_report).  The scores are cosine similarities in f32; a score that is
not finite is delivered as -2.  NO threshold is given here: what similarity separates two speakers depends on the checkpoint's speaker
encoder and is not measured.  The argument checks are pure Python and run without a device."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

TOP_MAX = 32                  # ZVX_SPK_TOP_MAX: the most places of one search
SLAB_ROWS = 512               # csrc/voicematch_kernels.h, SPK_SLAB: library rows per workgroup of the first launch of a top-k search
DIM_MAX = 2048


@dataclass(frozen=True)
class VoiceMatch:
    name: str
    index: int                # the row of the library at the time of the search
    score: float              # cosine similarity in f32; -2: not finite


@dataclass(frozen=True)
class VoiceReport:
    similarity: float         # cosine between the embedding of the delivered waveform and the one asked for
    frames: int               # mel frames the waveform was embedded from
    begin: int                # the trimmed window, in samples at the model's rate
    end: int

    def meets(self, min_similarity):
        """similarity >= min_similarity -- the caller's threshold; none is given here"""
        return self.similarity >= float(min_similarity)

    def __str__(self):
        return f"similarity {self.similarity:.4f} over {self.frames} frames (samples {self.begin} .. {self.end})"


def check_dim(dim):
    dim = int(dim)
    if dim < 4 or dim > DIM_MAX or dim % 4:
        raise ValueError(f"dim {dim} must be a multiple of 4 in [4, {DIM_MAX}]")
    return dim


def rows_2d(embeddings, dim, what="embeddings"):
    """[n][dim], [n][1][dim] or one [dim] -> float32 [n][dim]; ValueError names the width"""
    e = np.asarray(embeddings, np.float32)
    if e.ndim == 3 and e.shape[1] == 1:
        e = e[:, 0, :]
    if e.ndim == 1:
        e = e[None, :]
    if e.ndim != 2 or e.shape[1] != dim:
        raise ValueError(f"{what} of shape {tuple(np.shape(embeddings))} are not [n][{dim}]")
    return np.ascontiguousarray(e)


class VoiceLibrary:
    """Enrolled voices: one device buffer of f32 rows [capacity][dim] on `ctx`'s device, of which the first len(self) are in use, and the
    host list of their names.  The buffer grows by doubling (a device-to-device copy); rows written by ``enroll`` never visit the host.
    It belongs to its context and must be closed (or collected) before it."""

    def __init__(self, ctx, dim=None, capacity=1024):
        self._ctx = ctx
        self.dim = check_dim(ctx.hidden if dim is None else dim)
        if int(capacity) < 1:
            raise ValueError(f"capacity {capacity} must be at least 1")
        self._cap = int(capacity)
        self._names = []
        self._index = {}
        self._ptr = ctx.dev_alloc(self._cap * self.dim * 4)

    # ---- host state ---------------------------------------------------------------------------------------------------
    def __len__(self):
        return len(self._names)

    @property
    def names(self):
        return list(self._names)

    @property
    def capacity(self):
        return self._cap

    @property
    def ptr(self):
        """the device address of row 0 (it changes when the library grows)"""
        return self._ptr

    def _row_ptr(self, i):
        return self._ptr + int(i) * self.dim * 4

    def _check_new(self, names):
        names = [str(n) for n in names]
        seen = set()
        for n in names:
            if n in self._index or n in seen:
                raise ValueError(f"voice {n!r} is already in the library")
            seen.add(n)
        return names

    def _reserve(self, n):
        """room for n more rows"""
        need = len(self._names) + n
        if need <= self._cap:
            return
        cap = self._cap
        while cap < need:
            cap *= 2
        new = self._ctx.dev_alloc(cap * self.dim * 4)
        if self._names:
            self._ctx.dev_copy(new, self._ptr, len(self._names) * self.dim * 4)
        self._ctx.dev_free(self._ptr)
        self._ptr, self._cap = new, cap

    def _append(self, names):
        for n in names:
            self._index[n] = len(self._names)
            self._names.append(n)

    # ---- filling ------------------------------------------------------------------------------------------------------
    def add(self, names, embeddings):
        """host embeddings [n][dim] or [n][1][dim] under `names` -> the rows they took"""
        e = rows_2d(embeddings, self.dim)
        names = self._check_new(names)
        if len(names) != e.shape[0]:
            raise ValueError(f"{len(names)} names for {e.shape[0]} embeddings")
        if not names:
            return []
        self._reserve(len(names))
        first = len(self._names)
        self._ctx.dev_from_host(self._row_ptr(first), e)
        self._append(names)
        return list(range(first, first + len(names)))

    def enroll(self, names, clips, sampling_rate=None, **trim):
        """reference clips (1-D float waveforms at sampling_rate Hz; None: the model's) -> embeddings written by zvx_spkemb_wav straight
        into the library's rows.  trim: Context.spkemb_wav's keywords (frame, hop, top_db, keep, max_samples).  The width must be the
        model's.  -> (rows, begin, end, frames)"""
        names = self._check_new(names)
        clips = [np.asarray(c, np.float32).reshape(-1) for c in clips]
        if len(names) != len(clips):
            raise ValueError(f"{len(names)} names for {len(clips)} clips")
        if self.dim != self._ctx.hidden:
            raise ValueError(f"enroll: the library's width {self.dim} is not the model's {self._ctx.hidden}")
        if not names:
            return [], np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32)
        self._reserve(len(names))
        first = len(self._names)
        n = np.array([len(c) for c in clips], np.int32)
        nmax = max(int(n.max()), 1)
        x = np.zeros((len(clips), nmax), np.float32)
        for b, c in enumerate(clips):
            x[b, :n[b]] = c
        rows = self._ctx.dev_alloc(x.nbytes)
        try:
            self._ctx.dev_from_host(rows, x)
            begin, end, frames = self._ctx.spkemb_wav_device(rows, n, nmax, self._row_ptr(first), sampling_rate, **trim)
        finally:
            self._ctx.dev_free(rows)
        self._append(names)
        return list(range(first, first + len(names))), begin, end, frames

    def remove(self, name):
        """the last row moves into the hole: the library stays dense, the indices of the other rows stay"""
        name = str(name)
        if name not in self._index:
            raise ValueError(f"voice {name!r} is not in the library")
        i, last = self._index.pop(name), len(self._names) - 1
        if i != last:
            self._ctx.dev_copy(self._row_ptr(i), self._row_ptr(last), self.dim * 4)
            moved = self._names[last]
            self._names[i] = moved
            self._index[moved] = i
        self._names.pop()

    # ---- searching ----------------------------------------------------------------------------------------------------
    def _check_top(self, top):
        top = int(top)
        if top < 1 or top > TOP_MAX or top > len(self._names):
            raise ValueError(f"top {top} must lie in [1, min({len(self._names)} voices, {TOP_MAX})]")
        return top

    def match(self, queries, top=5):
        """host queries [B][dim] (or [B][1][dim], or one [dim]) -> per query the `top` best voices, a list of VoiceMatch by descending
        score (ascending row among equal scores)"""
        q = rows_2d(queries, self.dim, "queries")
        top = self._check_top(top)
        score, index = self._ctx.spk_topk(q, self._ptr, len(self._names), top, self.dim)
        return [[VoiceMatch(self._names[int(i)], int(i), float(s)) for s, i in zip(score[b], index[b])] for b in range(q.shape[0])]

    def screen(self, queries, min_score):
        """per query the voices that score at or above min_score (the caller's threshold), best first: duplicates at enrolment, or
        voices that must not be cloned.  Every row is scored (zvx_spk_score)."""
        q = rows_2d(queries, self.dim, "queries")
        if not self._names:
            return [[] for _ in range(q.shape[0])]
        score = self._ctx.spk_score(q, self._ptr, len(self._names), self.dim)
        out = []
        for b in range(q.shape[0]):
            hit = np.flatnonzero(score[b] >= np.float32(min_score))
            hit = hit[np.lexsort((hit, -score[b][hit].astype(np.float64)))]
            out.append([VoiceMatch(self._names[int(i)], int(i), float(score[b][i])) for i in hit])
        return out

    # ---- keeping ------------------------------------------------------------------------------------------------------
    def embeddings(self):
        """a copy of the rows in use on the host, float32 [len][dim]"""
        if not self._names:
            return np.zeros((0, self.dim), np.float32)
        return self._ctx.dev_to_host(self._ptr, (len(self._names), self.dim), np.float32)

    def save(self, path):
        """names and f32 rows as an .npz (written to exactly `path`)"""
        with open(path, "wb") as f:
            np.savez(f, names=np.array(self._names, dtype=np.str_), embeddings=self.embeddings())

    @classmethod
    def load(cls, ctx, path, capacity=None):
        with np.load(path, allow_pickle=False) as z:
            names, e = [str(n) for n in z["names"]], np.asarray(z["embeddings"], np.float32)
        if e.ndim != 2 or e.shape[0] != len(names):
            raise ValueError(f"{path}: {len(names)} names for embeddings of shape {e.shape}")
        lib = cls(ctx, dim=e.shape[1], capacity=max(len(names), 1) if capacity is None else capacity)
        lib.add(names, e)
        return lib

    def close(self):
        if getattr(self, "_ptr", None) and getattr(self._ctx, "_h", None):
            self._ctx.dev_free(self._ptr)
        self._ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
