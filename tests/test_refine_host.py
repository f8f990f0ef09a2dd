"""The pure helpers of the refine driver (monohair_amd/pmvo.py): the chunk / rank-slice rule, the schedule of the loss
launches of the smoothing chain, and the background writer of refine/*.npy.  No GPU."""
import numpy as np
import pytest

from monohair_amd.refine import _Writer, _chunk_slices, _loss_groups, _row_offsets

SIZES = (1, 4999, 5000, 5001, 10000, 16901)
RANKS = (1, 2, 3, 7)


def ceil_div(a, b):
    return (a + b - 1) // b


@pytest.mark.parametrize("ranks", RANKS)
@pytest.mark.parametrize("n_all", SIZES)
def test_chunk_slices_follow_the_rule(n_all, ranks):
    """`step = n_all // chunk + 1` chunks (PMVO.py:603); slice k of a chunk [lo, hi) is [lo + k*s, lo + (k+1)*s) cut at hi with
    s = ceil((hi-lo)/ranks): restated here, chunk by chunk."""
    chunk = 5000
    per_rank = [_chunk_slices(n_all, chunk, ranks, r) for r in range(ranks)]
    step = n_all // chunk + 1
    for r in range(ranks):
        assert len(per_rank[r]) == step
    for i in range(step):
        lo, hi = i * chunk, min(i * chunk + chunk, n_all)
        s = ceil_div(hi - lo, ranks)
        at = lo
        for r in range(ranks):
            got = per_rank[r][i]
            want_a, want_b = min(lo + r * s, hi), min(lo + r * s + s, hi)
            assert tuple(int(v) for v in got) == (lo, hi, s, want_a, want_b), (i, r, got)
            # disjoint, in rank order, none longer than s
            assert got[3] == at and got[3] <= got[4] <= hi and got[4] - got[3] <= s
            at = got[4]
        assert at == hi                                   # the slices cover [lo, hi) exactly


@pytest.mark.parametrize("ranks", RANKS)
@pytest.mark.parametrize("n_all", (5000, 10000))
def test_chunk_slices_trailing_chunk_of_no_points(n_all, ranks):
    for r in range(ranks):
        lo, hi, s, a, b = _chunk_slices(n_all, 5000, ranks, r)[-1]
        assert lo == hi == n_all and s == 0 and a == b == n_all
    assert len(_chunk_slices(n_all, 5000, ranks, 0)) == n_all // 5000 + 1


@pytest.mark.parametrize("ranks", RANKS)
@pytest.mark.parametrize("n_all", SIZES)
def test_row_offsets_are_prefix_sums_of_the_slice_lengths(n_all, ranks):
    total = 0
    for r in range(ranks):
        slices = _chunk_slices(n_all, 5000, ranks, r)
        row_of = _row_offsets(slices)
        assert len(row_of) == len(slices) + 1 and row_of[0] == 0
        acc = 0
        for i, (_, _, _, a, b) in enumerate(slices):
            assert row_of[i] == acc
            acc += b - a
        assert row_of[-1] == acc
        total += acc
    assert total == n_all                                 # every point is owned by exactly one rank
    assert _row_offsets(_chunk_slices(n_all, 5000, 1, 0))[:-1] == [i * 5000 for i in range(n_all // 5000 + 1)]


def test_loss_groups_cover_the_chunks_in_2_4_8_8():
    for step in range(1, 65):
        closes = _loss_groups(step)
        assert closes == sorted(set(closes)) and closes[-1] == step - 1 and 0 <= closes[0]
        sizes = [c - p for c, p in zip(closes, [-1] + closes[:-1])]      # contiguous groups (p, c], covering [0, step)
        assert sum(sizes) == step and min(sizes) >= 1
        want = [2, 4] + [8] * len(sizes)
        assert sizes[:-1] == want[:len(sizes) - 1]
        assert sizes[-1] <= want[len(sizes) - 1]


def test_loss_groups_of_the_headline_and_the_golden():
    """step = 58: the 287 696 points of the headline scene -- derived by hand from the loop this schedule came from;
    step = 4: the 16 901 points of the multi-chunk golden."""
    assert _loss_groups(58) == [1, 5, 13, 21, 29, 37, 45, 53, 57]
    assert _loss_groups(4) == [1, 3]


def test_writer_writes_what_it_was_given(tmp_path):
    rng = np.random.default_rng(0)
    arrays = {"a": rng.normal(size=(1000, 3)).astype(np.float32), "b": rng.normal(size=(7,)),
              "c": np.zeros((0, 3), np.float32), "d": np.array([np.nan, 1.0], np.float32)}
    w = _Writer()
    w.save(*[(str(tmp_path / (k + ".npy")), v) for k, v in arrays.items() if k in "ab"])       # one batch of two jobs
    for k in "cd":                                                                              # and two of one
        w.save((str(tmp_path / (k + ".npy")), arrays[k]))
    w.join()
    w.join()                                              # twice is harmless
    for k, v in arrays.items():
        got = np.load(tmp_path / (k + ".npy"))
        assert got.dtype == v.dtype and got.shape == v.shape and np.array_equal(got, v, equal_nan=True)


def test_writer_waits_for_the_event_of_a_job(tmp_path):
    class Event:
        def synchronize(self):
            filled[:] = 7.0

    filled = np.zeros(5, np.float32)
    w = _Writer()
    w.save((str(tmp_path / "f.npy"), filled, Event()), (str(tmp_path / "g.npy"), filled, None))
    w.join()
    assert np.array_equal(np.load(tmp_path / "f.npy"), np.full(5, 7.0, np.float32))
    assert np.array_equal(np.load(tmp_path / "g.npy"), np.full(5, 7.0, np.float32))


def test_writer_raises_the_first_error_on_join(tmp_path):
    w = _Writer()
    w.save((str(tmp_path / "first.npy"), np.arange(3)), (str(tmp_path / "no_such_directory" / "x.npy"), np.arange(3)),
           (str(tmp_path / "after.npy"), np.arange(3)))
    with pytest.raises(FileNotFoundError) as e:
        w.join()
    assert "no_such_directory" in str(e.value)
    assert (tmp_path / "first.npy").exists()
    assert not (tmp_path / "after.npy").exists()          # no job runs silently past the error
    w.join()                                              # the error was delivered: nothing more to raise


def test_writer_drops_a_batch_that_starts_after_an_error(tmp_path):
    w = _Writer()
    w.save((str(tmp_path / "no_such_directory" / "x.npy"), np.arange(3)))
    w.threads[0].join()                                   # (the failed batch is over; its error waits for join())
    w.save((str(tmp_path / "late.npy"), np.arange(3)))
    with pytest.raises(FileNotFoundError):
        w.join()
    assert not (tmp_path / "late.npy").exists()


def test_writer_that_is_not_enabled_writes_nothing(tmp_path):
    w = _Writer(enabled=False)                            # (a rank other than 0)
    w.save((str(tmp_path / "x.npy"), np.arange(3)))
    w.join()
    assert not (tmp_path / "x.npy").exists()


def test_a_process_that_fails_without_joining_the_writer_still_ends(tmp_path):
    """An error between save() and join() -- a failed launch in the shell stage, say -- must not leave a worker waiting for
    more jobs: the process writes what was queued, prints its traceback and ends."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import numpy as np\n"
            "from monohair_amd.refine import _Writer\n"
            "w = _Writer()\n"
            "w.save((%r, np.arange(5)))\n"
            "raise RuntimeError('after save, before join')\n") % (root, str(tmp_path / "queued.npy"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "after save, before join" in r.stderr, r.stderr[-500:]
    assert np.array_equal(np.load(tmp_path / "queued.npy"), np.arange(5))
