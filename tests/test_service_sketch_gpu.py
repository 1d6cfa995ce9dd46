"""The per-service latency sketch on the GPU: isim_service_sketch_device and isim_service_sketch
against isim_service_sketch_host, word for word with the header and at s in {0, 3, 7}, on synthetic spans
uploaded as one list entry (span counts around a wave, segments around the short tier's bound and around a
chunk, a short and a long service in one call, 64 lanes on one word and on 64 words, values around every bin's
lower bound, one code only, refused spans, a truncated list, an offset span pointer); a dirty workspace,
guards on both sides of the table, two calls into one table, a captured graph; and DesHandler.service_sketch
over two batches of the overloaded tree against DesHandler.service_quantiles of each."""
import numpy as np
import pytest

import isim
from isim import native
from isim.service_quantiles import CHUNK
from isim.service_sketch import (SHORT, service_sketch_device, service_sketch_table_words,
                                 service_sketch_workspace_bytes)

from test_service_quantiles_gpu import synth, tree
from test_service_sketch import bins_of, make_spans, services

pytestmark = pytest.mark.gpu

SUB_BITS = [0, 3, 7]
M64 = (1 << 64) - 1
GUARD = 64                                   # words of 0xA5 on either side of the table
A5 = np.uint64(0xA5A5A5A5A5A5A5A5)


class Call:
    """The device buffers of calls over uploaded spans: a 0xA5 workspace, a zeroed table between 0xA5 guards."""

    def __init__(self, h, s, spans, cap_spans=None, written_spans=None, skip=0):
        import torch
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64).ravel().copy()).to("cuda")  # noqa: E731
        self.h, self.s = h, s
        self.cap = len(spans) if cap_spans is None else cap_spans
        end = len(spans) if written_spans is None else written_spans
        # `skip` records of padding in front: the span pointer is then inside its buffer (16-byte aligned still)
        pad = np.full(64 * skip, 0xA5, np.uint8).view(isim.DES_SPAN_DTYPE)
        self.spans = up(np.concatenate([pad, spans])) if len(spans) + skip else torch.zeros(8, dtype=torch.int64, device="cuda")
        self.d_spans = self.spans.data_ptr() + 64 * skip
        self.off, self.info = up(np.array([0, end], np.uint64)), up(np.array([end, 1, 1, 1, 1], np.uint64))
        self.words = service_sketch_table_words(h, s)
        self.buf = torch.full((self.words + 2 * GUARD,), int(A5.astype(np.int64)), dtype=torch.int64, device="cuda")
        self.buf[GUARD:GUARD + self.words] = 0
        self.ws_bytes = service_sketch_workspace_bytes(h, self.cap)
        self.ws = torch.full((self.ws_bytes // 8 + 1,), int(A5.astype(np.int64)), dtype=torch.int64, device="cuda")

    def run(self, stream=None):
        import torch
        st = torch.cuda.current_stream().cuda_stream if stream is None else stream
        service_sketch_device(self.h, self.s, self.off.data_ptr(), self.d_spans, self.cap, self.info.data_ptr(),
                              self.buf.data_ptr() + 8 * GUARD, self.ws.data_ptr(), self.ws_bytes, st)
        return self

    def table(self):
        import torch
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy().view(np.uint64)
        assert np.all(b[:GUARD] == A5) and np.all(b[-GUARD:] == A5), "a guard word was written"
        return b[GUARD:-GUARD].copy()


def same_as_host(h, s, spans, want_spans=None, **kw):
    got = Call(h, s, spans, **kw).run().table()
    want = isim.service_sketch_host(h, spans if want_spans is None else want_spans, s)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:6], got[bad[:6]], want[bad[:6]])
    return got


@pytest.mark.parametrize("s", SUB_BITS)
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_span_counts(gpu, n, s):
    h = services(3)
    spans = synth([n // 3, n - n // 3 - n // 4, n // 4], seed=n)
    t = same_as_host(h, s, spans)
    assert list(t[-2:]) == [n, 0]
    assert np.array_equal(isim.service_sketch(h, spans, s), t)       # the synchronous entry point
    if n == 65:
        more = synth([40, 50, 45], seed=3)
        same_as_host(h, s, more, want_spans=more[:n], written_spans=n)        # a longer buffer, n written
        same_as_host(h, s, more[:n], written_spans=n + 70)                   # off[written] above cap_spans: truncated
        assert not Call(h, s, more, cap_spans=0).run().table().any()         # cap_spans 0 touches nothing
        same_as_host(h, s, more, skip=3)                                     # an offset span pointer


@pytest.mark.parametrize("s", SUB_BITS)
def test_truncation_and_an_offset_pointer_reach_a_long_segment(gpu, s):
    """The cases of test_span_counts where service 0 is long and in two chunks among the spans that count."""
    h = services(3)
    more = synth([CHUNK + 700, 40, SHORT + 30], seed=37)
    n = CHUNK + 300
    assert int((more[:n]["service"] == 0).sum()) > SHORT and int((more["service"] == 0).sum()) > CHUNK
    same_as_host(h, s, more, want_spans=more[:n], written_spans=n)        # a longer buffer, n written
    same_as_host(h, s, more[:n], written_spans=n + 70)                   # off[written] above cap_spans: truncated
    same_as_host(h, s, more, want_spans=more[:n], cap_spans=n)           # cap_spans below what the list claims
    assert not Call(h, s, more, cap_spans=0).run().table().any()         # cap_spans 0 touches nothing
    same_as_host(h, s, more, skip=3)                                     # an offset span pointer


TIERS = {
    "short_bound_minus_1": [SHORT - 1], "short_bound": [SHORT], "short_bound_plus_1": [SHORT + 1],
    "chunk_minus_1": [CHUNK - 1], "chunk": [CHUNK], "chunk_plus_1": [CHUNK + 1], "two_chunks_plus_1": [2 * CHUNK + 1],
    "short_and_long": [SHORT - 3, 0, CHUNK + 904, 17, SHORT + 1, 0, 1],
}


@pytest.mark.parametrize("s", SUB_BITS)
@pytest.mark.parametrize("name", list(TIERS))
def test_segments_around_the_tiers(gpu, name, s):
    lengths = TIERS[name]
    t = same_as_host(services(len(lengths)), s, synth(lengths, seed=7))
    per = t[:-2].reshape(len(lengths), 3, -1).sum(axis=2)
    assert [list(map(int, r)) for r in per] == [[n] * 3 for n in lengths] and list(t[-2:]) == [sum(lengths), 0]


def constant(rng, n):
    return np.full(n, 1000, np.uint64), np.full(n, 24, np.uint64)


@pytest.mark.parametrize("s", SUB_BITS)
@pytest.mark.parametrize("n", [64, SHORT + 64], ids=["short", "long"])
def test_every_lane_on_one_word(gpu, n, s):
    t = same_as_host(services(2), s, synth([0, n], seed=1, values=constant, p500=0.0))
    assert sorted(int(x) for x in t[t != 0]) == [n] * 4        # three words and FOLDED


@pytest.mark.parametrize("s", SUB_BITS)
@pytest.mark.parametrize("reps", [1, (SHORT + 64) // 64], ids=["short", "long"])
def test_every_lane_on_another_bin(gpu, reps, s):
    """Every 64 consecutive spans have waits in 64 distinct bins (the powers of two, an octave each)."""
    spans = make_spans([(0, 1 << i, (1 << i) + 5, 0, 0) for i in range(64)] * reps)
    t = same_as_host(services(1), s, spans)
    assert np.count_nonzero(t[:bins_of(s)]) == 64 and int(t[:bins_of(s)].max()) == reps


@pytest.mark.parametrize("s", SUB_BITS)
@pytest.mark.parametrize("where", ["short", "long"])
def test_values_around_every_bins_lower_bound(gpu, where, s):
    """The wait takes lo - 1, lo and lo + 1 of every bin: in one long segment, or over short ones."""
    vals = []
    for b in range(bins_of(s)):
        lo, _ = isim.sketch_bounds(s, b)
        vals += [v for v in (lo - 1, lo, lo + 1) if 0 <= v <= M64]
    if where == "long":
        vals = vals * (SHORT // len(vals) + 1)
        assert len(vals) > SHORT
    ns = 1 if where == "long" else -(-len(vals) // SHORT)
    spans = make_spans([(0, v, v, 0 if where == "long" else i // SHORT, i & 1) for i, v in enumerate(vals)])
    same_as_host(services(ns), s, spans)


@pytest.mark.parametrize("s", SUB_BITS)
@pytest.mark.parametrize("p500", [0.0, 1.0], ids=["all_200", "all_500"])
def test_one_code_only(gpu, p500, s):
    lengths = [SHORT + 200, 90]
    t = same_as_host(services(2), s, synth(lengths, seed=11, p500=p500))
    blocks = t[:-2].reshape(2, 3, 2, -1)
    assert not blocks[:, :, 0 if p500 else 1].any() and int(blocks[:, :, 1 if p500 else 0].sum()) == 3 * sum(lengths)


@pytest.mark.parametrize("s", SUB_BITS)
def test_refused_spans_are_refused_as_on_the_host(gpu, s):
    h = services(5)
    spans = synth([CHUNK + 100, 300, 0, SHORT + 5, 77], seed=19)
    m = len(spans)
    bad = spans.copy()
    pick = np.random.default_rng(5).permutation(m)
    bad["service"][pick[:100]] = 5
    bad["service"][pick[100:200]] = 0xFFFFFFFF
    bad["start_ns"][pick[200:300]] = bad["arrival_ns"][pick[200:300]] - 1
    bad["finish_ns"][pick[300:400]] = bad["start_ns"][pick[300:400]] - 1
    bad["start_ns"][pick[400:450]] = M64
    t = same_as_host(h, s, bad)
    assert int(t[-2 + native.SVQ_H_REFUSED]) >= 400 and int(t[-2]) + int(t[-1]) == m
    keep = np.ones(m, bool)
    keep[pick[:450]] = False
    assert np.array_equal(t[:-2], isim.service_sketch_host(h, bad[keep], s)[:-2])   # a refused span adds to nothing else


MIXED = [CHUNK + 904, 0, 17, SHORT + 1, 200]


@pytest.mark.parametrize("s", SUB_BITS)
def test_two_calls_add_and_merge(gpu, s):
    h = services(len(MIXED))
    first, second = synth(MIXED, seed=23), synth(MIXED[::-1], seed=29)
    once = isim.service_sketch_host(h, first, s)
    # the same spans twice, over the workspace the first call left
    c = Call(h, s, first)
    assert np.array_equal(c.run().run().table(), 2 * once)
    # two lists into one table against the host's merge; the second call has buffers of its own
    a, b = Call(h, s, first), Call(h, s, second)
    a.run()
    b.buf = a.buf
    want = isim.service_sketch_merge(h, s, once.copy(), isim.service_sketch_host(h, second, s))
    assert np.array_equal(b.run().table(), want)
    assert np.array_equal(isim.service_sketch(h, second, s, out=isim.service_sketch(h, first, s)), want)


@pytest.mark.parametrize("s", SUB_BITS)
def test_the_call_captured_in_a_graph(gpu, s):
    import torch
    h = services(len(MIXED))
    spans = synth(MIXED, seed=31 + s)       # a handler, sub_bits and sizes this process has not launched with
    c = Call(h, s, spans)
    once = isim.service_sketch_host(h, spans, s)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            c.run(st.cuda_stream)           # captured, not run
        for k in range(1, 4):
            g.replay()
            st.synchronize()
            assert np.array_equal(c.table(), k * once)      # k host folds
            c.ws.fill_(-1)                  # another dirt before the next replay
    torch.cuda.synchronize()


def test_handler_service_sketch_over_two_batches(gpu):
    from test_des_gpu import DesCase
    c = DesCase(tree(3, 3), 700_000, flags=native.FLAG_DYNAMIC)      # 13 services, overloaded
    n, s, q = 3000, 3, (0.5, 0.99, 1.0)
    ns = c.h.info.n_services
    sk = isim.ServiceSketch(c.h, s)
    totals = []
    for k, begin in enumerate((1000, 1000 + n)):
        if k == 0:
            one = c.d.service_sketch(begin, n, s)                   # a table of its own, merged on the host
            sk.merge(one)
        else:
            before = sk.flat.copy()
            assert c.d.service_sketch(begin, n, s, into=sk) is sk   # added into the first batch's
            one = isim.ServiceSketch(c.h, s, sk.flat - before)
        exact = c.d.service_quantiles(begin, n, q)
        assert one.header == exact.header and one.header["refused"] == 0
        br = one.quantiles(q)
        for m in isim.MEASURE_NAMES:
            for cls in ("all", "200", "500"):
                d, v = br[m][cls], exact.values[m][cls]
                assert np.array_equal(d["count"], exact.counts[cls])
                assert np.all(d["lo"] <= v) and np.all(v <= d["hi"]), (m, cls)
        totals.append(one.header["folded"])
    assert sk.header == {"folded": sum(totals), "refused": 0} and min(totals) > n
    # for every service and code the three measures hold the same number of spans
    per = sk.blocks.sum(axis=3)
    assert per.shape == (ns, 3, 2) and np.array_equal(per[:, 0], per[:, 1]) and np.array_equal(per[:, 0], per[:, 2])
    assert int(per[:, 0].sum()) == sum(totals)
    assert len(sk.worst("wait", 0.99, 3)) == 3 and sk.worst("wait", 0.99, 1)[0][1][1] > 0      # contended
    with pytest.raises(RuntimeError):
        c.d.service_sketch(1000, n, s, into=sk, cap_spans=totals[0] - 1)
    assert sk.header["folded"] == sum(totals)       # a batch that did not fit adds nothing
