"""GPU: monohair_amd/transfer.py on its own -- the named and the whole-array upload, the download, the stream registry, and
an object dropped with ring uploads in flight.  (The ring itself: test_edge_cases_gpu.py, upload_ring_wraps...)"""
import gc

import numpy as np
import pytest
import torch

from test_edge_cases_gpu import DEV, build

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pm():
    return build(24, 96, 80, 3)[1]


def host(t):
    return t.cpu().numpy()


def test_named_upload_grows_under_a_copy_in_flight_and_takes_a_dtype(pm):
    x, rng = pm.transfer, np.random.default_rng(0)
    arrs = [rng.standard_normal((n, 3)) for n in (3000, 7000, 10)]          # float64 in
    devs = [x.upload_named("a", a) for a in arrs]                           # no synchronisation: the buffer grows at the second
    b = rng.standard_normal((500, 3))
    dev_b = x.upload_named("b", b, np.float64)
    empty = x.upload_named("a", np.zeros((0, 3))), x.upload_named("b", np.zeros((0, 3)), np.float64)
    torch.cuda.synchronize()
    for a, d in zip(arrs, devs):
        assert d.dtype == torch.float32 and d.device == torch.device(DEV)
        assert np.array_equal(host(d), a.astype(np.float32))
    assert dev_b.dtype == torch.float64 and np.array_equal(host(dev_b), b)
    assert [(e.shape, e.dtype) for e in empty] == [((0, 3), torch.float32), ((0, 3), torch.float64)]


def test_whole_upload_in_two_parts_and_again_without_a_synchronisation(pm):
    x, rng = pm.transfer, np.random.default_rng(1)
    p1, p2 = rng.standard_normal((12000, 3)), rng.standard_normal((20000, 3))
    seen = []

    def after_head(dev):
        seen.append((dev, dev[:5000].clone()))       # queued behind the copy of the head rows, before the rest goes up

    d1, h1 = x.upload_whole(p1, head=5000, after_head=after_head)
    assert len(seen) == 1 and seen[0][0] is d1
    assert h1.dtype == np.float32 and np.array_equal(h1, p1.astype(np.float32))      # (valid until the next call)
    d2, h2 = x.upload_whole(p2, head=50000, after_head=after_head)                   # head > M: one part, then the callback
    assert len(seen) == 2 and seen[1][0] is d2
    assert np.array_equal(h2, p2.astype(np.float32))
    d3, h3 = x.upload_whole(p1, head=5000)                                           # no callback: one part
    e_dev, e_host = x.upload_whole(np.zeros((0, 3)))
    torch.cuda.synchronize()
    assert np.array_equal(host(seen[0][1]), p1[:5000].astype(np.float32))
    assert np.array_equal(host(d1), p1.astype(np.float32))
    assert np.array_equal(host(d2), p2.astype(np.float32)) and np.array_equal(host(seen[1][1]), p2[:5000].astype(np.float32))
    assert np.array_equal(host(d3), p1.astype(np.float32)) and np.array_equal(h3, p1.astype(np.float32))
    assert len(seen) == 2
    assert e_dev.shape == (0, 3) and e_dev.dtype == torch.float32 and e_host.shape == (0, 3) and e_host.dtype == np.float32


@pytest.mark.parametrize("after", ["event", "stream"])
def test_download_waits_for_its_producer_and_returns_the_event_that_ends_it(pm, after):
    x = pm.transfer
    side, cp = x.stream("test_side"), x.stream("test_copy")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        a = torch.randn((5000, 3), device=DEV)
        for _ in range(20):                          # (some work in front of the values the copies read)
            a = a * 1.0001 + 0.5
        b = a[:, 0] * 2
        c = b > 0
        ev = torch.cuda.Event()
        ev.record(side)
    got, done = x.download(cp, ev if after == "event" else side, [a, b, c])
    done.synchronize()
    got = [g.copy() for g in got]                    # what the arrays hold once the returned event has passed
    torch.cuda.synchronize()
    assert [g.dtype for g in got] == [np.float32, np.float32, np.bool_]
    for g, t in zip(got, (a, b, c)):
        assert g.shape == tuple(t.shape) and np.array_equal(g, host(t))
    rows = [x.pinned_like(t) for t in (a, b, c)]     # the form that fills rows of arrays the caller keeps
    _, done = x.download(cp, None, [t[100:200] for t in (a, b, c)], into=[r[100:200] for r in rows])
    done.synchronize()
    for r, t in zip(rows, (a, b, c)):
        assert np.array_equal(r.numpy()[100:200], host(t)[100:200])


def test_an_object_dropped_with_uploads_in_flight_drains_them_first():
    from monohair_amd import synth

    cand = synth.candidate_points(res=32, seed=1)
    rng = np.random.default_rng(2)
    chunks = [np.ascontiguousarray(cand[rng.choice(len(cand), int(rng.integers(1, 400)))]) for _ in range(40)]

    def run(pm):
        st, outs = pm.side_streams(2), []
        for i, c in enumerate(chunks):               # no synchronisation
            with torch.cuda.stream(st[i % 2]):
                outs.append(pm.forward(c))
        return outs

    pm1 = build(24, 96, 80, 3)[1]
    outs = run(pm1)
    del pm1
    gc.collect()
    torch.cuda.synchronize()
    pm2 = build(24, 96, 80, 3)[1]
    ref = run(pm2)
    torch.cuda.synchronize()
    for c, got, want in zip(chunks, outs, ref):
        assert np.array_equal(host(got[0]), c.astype(np.float32))
        for g, w in zip(got, want):
            assert np.array_equal(host(g), host(w), equal_nan=True)


def test_side_streams_are_created_once_and_extended(pm):
    two = pm.side_streams(2)
    assert len(two) == 2 and two[0].cuda_stream != two[1].cuda_stream
    again = pm.side_streams(2)
    assert all(a is b for a, b in zip(two, again))
    three = pm.side_streams(3)
    assert len(three) == 3 and three[0] is two[0] and three[1] is two[1]
    assert len({s.cuda_stream for s in three}) == 3
    assert pm.transfer.stream("copy") is pm.transfer.stream("copy")
