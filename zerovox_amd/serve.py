"""Continuous batching of stream sessions (include/zvx.h: zvx_stream_next_many): many listeners, one vocoder run per step.

A ``StreamBatcher`` keeps the open sessions of ONE context.  ``open`` adds a session at any time, ``step`` advances the open sessions by one
piece each with a single ``Context.stream_next_many`` and hands back what they produced, sessions that report done are closed and dropped.
Every session's pieces are, bit for bit and piece by piece, the pieces the same session hands out when it is stepped alone.

The scheduling is plain Python on top of three context methods (``stream_open``, ``stream_next_many`` and, per session, ``close`` /
``done``), so a stand-in context tests it without a device."""
from __future__ import annotations

MAX_SESSIONS = 64                                    # ZVX_STREAM_MANY_MAX_SESSIONS
MAX_ROWS = 256                                       # ZVX_STREAM_MANY_MAX_ROWS


class _Entry:
    __slots__ = ("id", "stream", "left", "cpc", "waited")

    def __init__(self, id_, stream, chunks, cpc):
        self.id, self.stream, self.left, self.cpc, self.waited = id_, stream, chunks, cpc, 0

    def rows(self):
        """the rows this session's next group brings: min(chunks_per_call, chunks left)"""
        return max(1, min(self.cpc, self.left))


class StreamBatcher:
    """open(mel, **stream_open keywords) -> id; step() -> [(id, piece, done), ...]; close(id); len().

    A step takes every open session when their groups fit ``max_rows`` rows (at most 256) and 64 sessions.  When they do not, it takes the
    sessions that have waited longest first -- ties in the order they were opened -- and skips a session whose group no longer fits; the
    rest wait for the next step.  A session that was left out has then waited longer than every session that was served, so it is among
    the first of the next step: no session starves.  Sessions opened between two steps simply take part in the next."""

    def __init__(self, ctx, max_rows=MAX_ROWS):
        if not 1 <= int(max_rows) <= MAX_ROWS:
            raise ValueError(f"StreamBatcher: max_rows {max_rows} outside 1 .. {MAX_ROWS}")
        self._ctx, self._max_rows, self._open, self._next_id = ctx, int(max_rows), {}, 0

    def __len__(self):
        return len(self._open)

    def open(self, mel=None, frames=0, *, chunk_frames, chunks_per_call=1, **kw):
        """opens a session on ``mel`` (Context.stream_open's arguments) -> its id.  Every keyword is forwarded: denoise / bias / limit, and
        the stages of zvx_stream_open_ex, ``level=`` (Context.level_window's keywords) and ``watermark=`` (a watermark.params(...) dict
        whose ``key`` is this session's) -- sessions of equal level parameters, and sessions whose watermark differs in the key alone,
        each cost one launch group per step.  A session whose group alone exceeds max_rows could never be scheduled: ValueError."""
        cpc = max(1, int(chunks_per_call))
        if mel is None:                                              # the context's mel, its length unknown here: every group counts as
            chunks = 1 << 62                                         # chunks_per_call rows (an upper bound; the budget stays safe)
        else:
            n = len(mel) if hasattr(mel, "__len__") else int(frames)     # (an int is a device pointer to `frames` rows)
            chunks = max(1, -(-n // max(1, int(chunk_frames))))
        if min(cpc, chunks) > self._max_rows:
            raise ValueError(f"StreamBatcher.open: a group of {min(cpc, chunks)} chunks exceeds max_rows {self._max_rows}")
        stream = self._ctx.stream_open(mel, frames, chunk_frames=chunk_frames, chunks_per_call=cpc, **kw)
        id_ = self._next_id
        self._next_id += 1
        self._open[id_] = _Entry(id_, stream, chunks, cpc)
        return id_

    def close(self, id_):
        """closes and drops a session before it is done (an unknown id: KeyError)"""
        self._open.pop(id_).stream.close()

    def _pick(self):
        """the sessions of the next step: longest wait first, within the row and session budgets"""
        picked, rows = [], 0
        for e in sorted(self._open.values(), key=lambda e: (-e.waited, e.id)):
            if len(picked) == MAX_SESSIONS:
                break
            if rows + e.rows() <= self._max_rows:
                picked.append(e)
                rows += e.rows()
        return picked

    def step(self):
        """one stream_next_many over the sessions of this step -> [(id, piece, done), ...] in the order they were stepped; pieces may be
        empty (a stage still filling its reach).  Sessions that report done are closed and dropped."""
        picked = self._pick()
        if not picked:
            return []
        pieces = self._ctx.stream_next_many([e.stream for e in picked])
        served = {e.id for e in picked}
        for e in self._open.values():
            e.waited = 0 if e.id in served else e.waited + 1
        out = []
        for e, piece in zip(picked, pieces):
            e.left -= e.rows()
            done = bool(e.stream.done)
            out.append((e.id, piece, done))
            if done:
                self.close(e.id)
        return out

    def close_all(self):
        for id_ in list(self._open):
            self.close(id_)
