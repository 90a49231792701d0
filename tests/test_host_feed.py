"""host_feed (the upload pipeline of the from-host prediction paths) without a device: the ledger of what is on the device, the
prefetch loop replayed over the plans the three paths produce, and StreamingPredictor.host_span_plan.  Host arithmetic only."""
import numpy as np
import pytest

STREAM_CASES = (   # (n samples, T, hop, windows per span); the last one is long enough for the ramp to take effect
    (160 * (800 + 400 * 7), 800, 400, 3),
    (160 * (800 + 400 * 5) + 160 * 173 + 55, 800, 400, 2),
    (160 * 500 + 7, 800, 400, 3),   # one padded window
    (160 * 100 + 3, 8, 4, 5),
    (160 * 2000 + 3, 8, 4, 256),
)


@pytest.fixture(scope="module")
def lib():
    from voice_activity_detection_amd import _lib, build

    build.build()
    return _lib.load()


def _union(ranges):
    """sorted disjoint ranges covering the same positions (touching ranges merged)"""
    out = []
    for a, b in sorted(r for r in ranges if r[1] > r[0]):
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return [tuple(r) for r in out]


def _size(ranges):
    return sum(b - a for a, b in ranges)


def test_ledger_hands_out_every_position_once():
    """Uploaded.missing over arbitrary request sequences (the tail first among them), against a set of positions: the pieces are
    disjoint, in order, inside the request, new, and together with what was there they are the request; the ranges stay sorted,
    disjoint and merged"""
    from voice_activity_detection_amd.host_feed import Uploaded

    rng = np.random.default_rng(11)
    sequences = [[(150, 200), (0, 60), (40, 120), (100, 200)],       # the tail first, then a prefix that grows into it
                 [(10, 20), (30, 40), (0, 50), (0, 50), (50, 50), (45, 70)],
                 [(5, 6), (6, 7), (4, 5), (0, 200)]]
    sequences += [[tuple(sorted(int(v) for v in rng.integers(0, 201, 2))) for _ in range(12)] for _ in range(200)]
    for seq in sequences:
        ledger, present = Uploaded(), set()
        for a, b in seq:
            pieces = ledger.missing(a, b)
            assert all(a <= lo < hi <= b for lo, hi in pieces), (seq, pieces)
            assert all(p[1] < q[0] for p, q in zip(pieces, pieces[1:])), (seq, pieces)   # in order, disjoint, not touching
            got = {i for lo, hi in pieces for i in range(lo, hi)}
            assert got == set(range(a, b)) - present, (seq, a, b, pieces)
            present |= got
            assert ledger.ranges == _union(ledger.ranges) and {i for lo, hi in ledger.ranges for i in range(lo, hi)} == present
        assert present == {i for a, b in seq for i in range(a, b)}


def _replay(needs):
    """HostFeed.chunks over `needs` with the ledger in place of the copies -> what each request copies, after checking: request c is
    what chunk c waits for, request c + 1 is already made then, what requests 0 .. c copy covers needs[c], a request copies at most
    one piece, no position is copied twice, everything needed is copied"""
    from voice_activity_detection_amd.host_feed import HostFeed, Uploaded

    class LedgerFeed(HostFeed):   # the loop and the ledger of the real feed; no stream, no buffer
        def __init__(self):
            self.uploaded, self.copies, self.current, self.waited = Uploaded(), [], self, None

        def request(self, a, b):
            self.copies.append(self.uploaded.missing(a, b))
            return len(self.copies) - 1   # the "event": which request it closes

        def wait_event(self, ev):   # (the feed's `current` stream is the feed itself here)
            self.waited = ev

    feed, consumed = LedgerFeed(), []
    for c in feed.chunks(needs):
        assert feed.waited == c and len(feed.copies) == min(c + 2, len(needs))
        arrived = _union(p for pieces in feed.copies[:c + 1] for p in pieces)
        a, b = needs[c]
        assert any(lo <= a and b <= hi for lo, hi in arrived), (c, needs[c], arrived)
        consumed.append(c)
    assert consumed == list(range(len(needs)))
    assert all(len(pieces) <= 1 for pieces in feed.copies), feed.copies
    flat = sorted(p for pieces in feed.copies for p in pieces)
    assert all(p[1] <= q[0] for p, q in zip(flat, flat[1:])), flat
    assert _size(flat) == _size(_union(needs))
    return feed.copies


def _prefix_and_tail_copies(needs):
    """the bookkeeping the paths had before the ledger: a prefix [0, uploaded) and, when the first need does not start at 0 (the short
    last span, taken first), a tail [tail_from, n)"""
    uploaded, tail_from, copies = 0, max(b for _, b in needs), []
    for c, (a, b) in enumerate(needs):
        if c == 0 and a > 0:
            copies.append([(a, b)])
            tail_from = a
        else:
            a, b = max(a, uploaded), min(b, tail_from)
            copies.append([(a, b)] if b > a else [])
            uploaded = max(uploaded, b)
    return copies


@pytest.mark.parametrize("ramp", [False, True])
def test_streaming_plans_replayed(lib, ramp):
    from voice_activity_detection_amd import StreamingPredictor

    for n, T, hop, per in STREAM_CASES:
        plan = StreamingPredictor.host_span_plan(n, T, hop, per, ramp)
        needs = [(first, first + count) for *_, first, count in plan]
        assert _replay(needs) == _prefix_and_tail_copies(needs), (n, T, hop, per)
        assert _union(needs) == [(0, n)]   # the spans read the whole recording


@pytest.mark.parametrize("rate,channels", [(16000, 1), (44100, 2)])
def test_reference_mode_plans_replayed(lib, rate, channels):
    """the needs are in raw frames (the feed's unit is the channel count); at 44.1 kHz they come through resample_span_samples, and
    each chunk's resampling step reads no frame beyond them"""
    from voice_activity_detection_amd import VADFromScratchPredictor
    from voice_activity_detection_amd.features import resample_length, resample_span_samples
    from voice_activity_detection_amd.predictor import window_offsets

    for half, jump in ((19, 9), (3, 1), (8, 4)):
        W = len(window_offsets(half, jump))
        for N, per in ((1001, 300), (1001, 250), (5000, 4096), (77, 1000), (2 * half, 100), (2 * half + 1, 100), (640, 160), (1, 10)):
            n = 160 * (N - 1) + 77
            n_in = n * rate // 16000
            assert resample_length(n_in, rate) == n
            n_plan, plan = VADFromScratchPredictor.host_upload_plan(n_in, rate, half, W, per)
            assert n_plan == n and [p[:4] for p in plan] == VADFromScratchPredictor.host_chunk_plan(N, half, W, per)
            needs = [(0, p[6]) for p in plan]
            assert _replay(needs) == _prefix_and_tail_copies(needs), (half, N, per)
            assert needs[-1] == (0, n_in)
            done16 = 0
            for f0, f1, g0, g1, first, count, have in plan:
                end16 = first + count
                if rate == 16000:
                    assert have == end16
                elif end16 > done16:
                    assert sum(resample_span_samples(n_in, rate, done16, end16 - done16)) <= have <= n_in
                done16 = max(done16, end16)


def test_host_span_plan(lib):
    """the spans tile [0, W) once; without ramp a short last span comes first and the rest are in order; with ramp the sizes are 32,
    64, ... below `per`, then `per`; each span's samples are span_samples of its frames"""
    from voice_activity_detection_amd import StreamingPredictor
    from voice_activity_detection_amd.features import span_samples

    ramped = 0
    for n, T, hop, per in STREAM_CASES:
        N = 1 + n // 160
        W = lib.savad_stream_window_count(N, T, hop)
        assert W >= 1
        for ramp in (False, True):
            plan = StreamingPredictor.host_span_plan(n, T, hop, per, ramp)
            in_order = sorted(plan)
            assert in_order[0][0] == 0 and in_order[-1][1] == W and all(p[1] == q[0] for p, q in zip(in_order, in_order[1:]))
            for lo, hi, f0, f1, first, count in plan:
                assert lo < hi and (f0, f1) == (hop * lo, min(N, hop * (hi - 1) + T))
                assert (first, count) == span_samples(n, f0, f1 - f0)
            sizes = [hi - lo for lo, hi, *_ in in_order]
            if ramp:
                assert plan == in_order
                want, step = [], 32
                while step < per and sum(want) < W:
                    want.append(step)
                    step *= 2
                ramped += len(want) > 1
                want += [per] * (len(sizes) - len(want))
                assert sizes[:-1] == want[:-1] and 0 < sizes[-1] <= want[-1]
            else:
                assert all(s == per for s in sizes[:-1]) and 0 < sizes[-1] <= per
                short_last = len(plan) > 1 and sizes[-1] < per
                assert plan == (in_order[-1:] + in_order[:-1] if short_last else in_order)
    assert ramped   # at least one case where the ramp has more than one step
    assert len(StreamingPredictor.host_span_plan(160 * 500 + 7, 800, 400, 3, False)) == 1
