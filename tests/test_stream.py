"""zerovox_amd.stream, no GPU needed: the reach planner's rules (every sample once and in order, latency R, the history kept, the support
condition of include/zvx.h restated on every planned window) for ReachPlanner itself and for the limiter's and the denoiser's planners
built for the same reach, and that the three stream functions run the one driver."""
import numpy as np
import pytest

from stream_util import supported
from zerovox_amd import denoiser as DN, limiter as LM, resample as RSM, stream as S

REACHES = [0, 1, 13, 231, 1023, 4095]
# R = 2 W + H is even (oversample 1, H = 0) or odd and at least 11 (H = 11): no limiter has a reach of 1
LIMITERS = {0: (0, 1), 13: (1, 2), 231: (110, 4), 1023: (506, 4), 4095: (2042, 4)}
PLANNERS = ([pytest.param(R, lambda R=R: S.ReachPlanner(R), id=f"reach-{R}") for R in REACHES]
            + [pytest.param(R, lambda a=a: LM.LimitPlanner(*a), id=f"limit-{R}") for R, a in LIMITERS.items()]
            + [pytest.param(R, lambda R=R: DN.DenoisePlanner(R + 1), id=f"denoise-{R}") for R in REACHES])


@pytest.mark.parametrize("R,make", PLANNERS)
def test_planner_emits_every_sample_once_with_latency_R(R, make):
    rng = np.random.default_rng(R)
    for sizes in ([1] * (2 * R + 52), [64] * 80, [int(v) for v in rng.integers(1, 3 * R + 5, 60)], [5 * R + 5]):
        p = make()
        assert p.R == R and (p.received, p.next_out, p.origin) == (0, 0, 0)
        received = emitted = origin = 0
        for k in sizes:
            o, b, c, keep = p.push(k, False)
            received += k
            assert o == origin and b == emitted and c >= 0                            # in order, nothing twice, nothing skipped
            emitted += c
            assert emitted == max(0, received - R), (sizes[:3], received)             # a non-last push emits up to received - R
            assert received - o <= k + 2 * R and supported(R, o, received - o, b, c, False)
            assert keep == max(o, emitted - R) and keep >= o                          # the history before next_out - R is dropped
            origin = keep
            assert (p.received, p.next_out, p.origin) == (received, emitted, origin)
        o, b, c, keep = p.push(0, True)                                               # push(0, True) flushes the rest
        assert o == origin and b == emitted and b + c == received and supported(R, o, received - o, b, c, True) and received - o <= 2 * R
    p = make()
    assert p.push(0, True) == (0, 0, 0, 0)                   # an empty stream
    assert list(S.stream_windows([], make(), None)) == []


def test_planners_record_their_own_parameters():
    p = LM.LimitPlanner(110, 4)
    assert (p.W, p.oversample, p.R) == (110, 4, 231) and LM.LimitPlanner(110, 1).R == 220
    p = DN.DenoisePlanner(1024)
    assert (p.n_fft, p.R) == (1024, 1023)


def test_every_stream_runs_the_one_driver(monkeypatch):
    assert LM.stream_limit is S.stream_windows and DN.stream_denoise is S.stream_windows and RSM.stream_windows is S.stream_windows
    seen = []

    def driver(chunks, planner, window_fn):
        seen.append(type(planner))
        return S.stream_windows(chunks, planner, window_fn)

    monkeypatch.setattr(RSM, "stream_windows", driver)
    x = np.arange(40, dtype=np.float32)
    pieces = list(RSM.stream_resample([x[:25], x[25:]], 22050, 22050, lambda s, o, b, n: s[b - o:b - o + n].copy()))
    assert seen == [RSM.StreamPlanner] and np.array_equal(np.concatenate(pieces), x)
