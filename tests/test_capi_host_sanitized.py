"""The host-only part of the C ABI (monohair_amd/csrc/capi_host.cpp: the MAT-v5 sparse writer and the strand gate) under
sanitizers, on the CPU: the file and tests/capi_host_main.cpp are compiled with the host compiler -- no HIP -- into a
stand-alone program, once with AddressSanitizer + UBSan and once with ThreadSanitizer.  The program must end with status 0
and without a report, and what it wrote is compared with numpy restatements of the documented behaviour: the inputs are made
here, no expected value comes from the library."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "monohair_amd", "csrc", "capi_host.cpp"), os.path.join(ROOT, "tests", "capi_host_main.cpp")]
MH_ERR_ARG = -1                                    # include/mh_pmvo.h

PREFIX = ((np.arange(136) * 37 + 1) & 255).astype(np.uint8)       # 136 bytes: the payload behind it is not page-aligned
SMALL_N = 1537                                     # three pages of doubles plus one element
SMALL_IDX = np.array([0, 1536, 5, 5, 700, 1536], dtype=np.int64)  # both ends, duplicates
SMALL_VAL = np.array([1.5, 2.5, 3.5, 4.5, 5.5, 6.5])
BIG_N, BIG_STORES = 6000, 5000                     # the writer threads from 4096 stores on
BIG_IDX = ((np.arange(BIG_STORES, dtype=np.int64) ** 2 * 31 + 7 * np.arange(BIG_STORES)) % BIG_N).astype(np.int64)
BIG_VAL = np.arange(BIG_STORES) + 0.25
X, Y, Z = 3, 4, 5
VOX = np.array([[0, 0, 0], [2, 3, 4], [1, 2, 3], [2, 3, 4]], dtype=np.int64)       # (x, y, z); the last row repeats the second
BAD_VOX = np.array([[1, 1, 1], [X, 0, 0]], dtype=np.int64)                         # x == X
ORI32 = (np.arange(12, dtype=np.float32).reshape(4, 3) + 0.5)
ORI64 = (np.arange(12, dtype=np.float64).reshape(4, 3) + 1) / 7.0                  # not float32 values
TOUCH = np.array([0, 0, 1, X * Y * Z - 1, 1000, -1], dtype=np.int64)               # repeated page, last element, out of range
STORE_IDX, STORE_VAL = np.array([7, 7, 58], dtype=np.int64), np.array([2.0, 3.0, 4.0])
W, H, D = 4, 3, 2                                  # the gate's volume (W, H, Z)
STRIDE = 8                                         # rows per strand in `pts`: more than any length below


def _gate_inputs():
    """mode 0 and mode 1 inputs of mh_strands_accept: (flag, pts [n, STRIDE, 3], first, len, seeds)"""
    a = (1.2, 1.3, 0.1)                            # voxel A = (1, 1, 0)
    junk = (0.5, 2.5, 1.5)                         # voxel (0, 2, 1): rows outside [first, first + len) hold it
    flag0 = np.zeros(W * H * D, dtype=np.float32)
    flag0[(1 * H + 2) * W + 3] = 3.0               # voxel (3, 2, 1) is full
    strands0 = [
        # (seed, first, points)
        ((3.2, 2.1, 1.0), 0, [(0.5, 0.5, 1.5)] * 6),                                          # seed voxel full: skipped
        ((0.5, 0.5, 0.5), 0, [(0.5, 0.5, 1.5)] * 4),                                          # 4 points: skipped
        ((0.5, 0.5, 0.5), 0, [a, (1.7, 1.9, 0.9), (-0.5, 0.2, 0.0), (W + 2.0, 1.0, 0.0), (2.5, 2.5, 1.5)]),   # A twice, clamps
        ((1.0, 1.0, 0.0), 2, [a, (2.5, 0.5, 0.5), (2.9, 0.1, 0.2), (3.5, 1.5, 0.5), (0.5, 0.5, 1.5)]),        # A again, first > 0
        ((0.1, 0.1, 0.1), 1, [a, a, a, (1.5, 0.5, 1.5), (1.5, 0.5, 1.5)]),                    # A reaches 3
        ((1.5, 1.5, 0.5), 0, [(0.5, 0.5, 1.5)] * 5),                                          # seeded in A, now full: skipped
    ]
    flag1 = np.full(W * H * D, 5.0, dtype=np.float32)
    flag1[(0 * H + 1) * W + 1] = 2.0
    strands1 = [((0.0, 0.0, 0.0), 0, []),                                                     # no points: skipped
                ((0.0, 0.0, 0.0), 3, [a, a, (3.5, 2.5, 1.5)])]
    out = []
    for flag, strands in ((flag0, strands0), (flag1, strands1)):
        n = len(strands)
        pts = np.tile(np.array(junk, dtype=np.float32), (n, STRIDE, 1))
        first = np.array([s[1] for s in strands], dtype=np.int32)
        length = np.array([len(s[2]) for s in strands], dtype=np.int32)
        for i, (_, f, p) in enumerate(strands):
            if p:
                pts[i, f:f + len(p)] = np.array(p, dtype=np.float32)
        out.append((flag, pts, first, length, np.array([s[0] for s in strands], dtype=np.float32)))
    return out


def _gate_np(flag, pts, first, length, seeds, mode):
    """include/mh_pmvo.h, mh_strands_accept: strands in order; mode 0 skips a strand whose seed voxel holds 3 or more or
    that has fewer than 5 points, and adds 1 to every distinct voxel of an accepted one; mode 1 keeps what has points and
    sets its voxels to 1.  A point's voxel: its coordinates truncated and clamped into the volume."""
    def voxel(p):
        v = np.clip(np.trunc(p).astype(np.int64), 0, [W - 1, H - 1, D - 1])
        return (v[..., 2] * H + v[..., 1]) * W + v[..., 0]

    flag, accepted = flag.copy(), np.zeros(len(length), dtype=np.uint8)
    for i in range(len(length)):
        if (mode == 0 and (flag[voxel(seeds[i])] >= 3 or length[i] < 5)) or (mode == 1 and length[i] <= 0):
            continue
        accepted[i] = 1
        q = voxel(pts[i, first[i]:first[i] + length[i]])
        if mode == 1:
            flag[q] = 1
        else:
            flag[np.unique(q)] += 1
    return flag, accepted


def _write_inputs(d):
    gate0, gate1 = _gate_inputs()
    arrays = {"prefix": PREFIX, "small_idx": SMALL_IDX, "small_val": SMALL_VAL, "small_nelem": np.array([SMALL_N], dtype=np.int64),
              "big_idx": BIG_IDX, "big_val": BIG_VAL, "big_nelem": np.array([BIG_N], dtype=np.int64),
              "grid_dims": np.array([X, Y, Z], dtype=np.int64), "vox": VOX, "bad_vox": BAD_VOX, "ori32": ORI32, "ori64": ORI64,
              "touch_idx": TOUCH, "store_idx": STORE_IDX, "store_val": STORE_VAL,
              "accept_whz": np.array([W, H, D], dtype=np.int64), "accept_stride": np.array([STRIDE], dtype=np.int64)}
    for tag, gate in (("acc0", gate0), ("acc1", gate1)):
        arrays.update({"%s_%s" % (tag, k): v for k, v in zip(("flag", "pts", "first", "len", "seeds"), gate)})
    for name, a in arrays.items():
        np.ascontiguousarray(a).tofile(os.path.join(d, name + ".bin"))


def _build_and_run(tmp, sanitize, what):
    cxx = os.environ.get("CXX") or shutil.which("g++") or "/opt/rocm/llvm/bin/clang++"
    d = str(tmp)
    exe = os.path.join(d, "capi_host_main")
    # the sanitizer runtimes linked statically (clang's default), so that the program does not depend on being loaded first
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libtsan"] if sanitize == "thread" else ["-static-libasan",
                                                                                                          "-static-libubsan"]
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=" + sanitize, "-fno-sanitize-recover=all", "-pthread",
                           "-o", exe] + static + SOURCES)
    _write_inputs(d)
    r = subprocess.run([exe, what], cwd=d, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, "exit status %d\n%s" % (r.returncode, r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    status = {}
    for line in open(os.path.join(d, "status.txt")):
        key, _, value = line.rstrip("\n").partition(" ")
        status[key] = value
    return d, status


@pytest.fixture(scope="module")
def asan(tmp_path_factory):
    return _build_and_run(tmp_path_factory.mktemp("capi_host_asan"), "address,undefined", "all")


def _mat(d, name):
    return open(os.path.join(d, name), "rb").read()


def _expect(nelem, idx, val):
    a = np.zeros(nelem)
    for i, v in zip(idx, val):                     # in order: later stores win
        a[i] = v
    return PREFIX.tobytes() + a.tobytes()


def test_write_sparse(asan):
    d, st = asan
    assert st["ws_small"] == "0" and st["ws_empty"] == "0"
    assert _mat(d, "ws_small.mat") == _expect(SMALL_N, SMALL_IDX, SMALL_VAL)
    assert _mat(d, "ws_empty.mat") == _expect(SMALL_N, [], [])
    assert int(st["ws_range"]) == MH_ERR_ARG and "out of range" in st["ws_range_error"]


def test_write_sparse_threads(asan):
    d, st = asan
    assert len(np.unique(BIG_IDX)) < BIG_STORES and BIG_STORES >= 4096
    assert st["ws_t1"] == "0" and st["ws_t4"] == "0"
    assert _mat(d, "ws_t1.mat") == _expect(BIG_N, BIG_IDX, BIG_VAL)
    assert _mat(d, "ws_t4.mat") == _mat(d, "ws_t1.mat")


def test_sparse_handle(asan):
    d, st = asan
    assert int(st["open_prefix4"]) == MH_ERR_ARG and st["open_prefix4_handle_null"] == "1" and st["close_null"] == "0"
    for key in ("occ_open", "occ_touch", "occ_store", "occ_store_voxels", "occ_close", "ori32_open", "ori32_touch",
                "ori32_store_voxels", "ori32_close", "ori64_open", "ori64_store_voxels", "ori64_close"):
        assert st[key] == "0", key
    assert int(st["ori32_bad_voxel"]) == MH_ERR_ARG
    plane = X * Y * Z
    assert _mat(d, "sp_occ_after_touch.bin") == _expect(plane, [], [])
    lin = VOX[:, 1] + Y * (VOX[:, 0] + X * VOX[:, 2])
    assert _mat(d, "sp_occ.mat") == _expect(plane, list(STORE_IDX) + list(lin), list(STORE_VAL) + [1.0] * len(lin))
    for name, ori in (("sp_ori32.mat", ORI32), ("sp_ori64.mat", ORI64)):
        idx = [l + c * plane for l, _ in zip(lin, ori) for c in range(3)]
        assert _mat(d, name) == _expect(3 * plane, idx, ori.astype(np.float64).reshape(-1)), name


def test_strands_accept(asan):
    d, st = asan
    gate0, gate1 = _gate_inputs()
    for tag, gate, mode in (("acc0", gate0, 0), ("acc1", gate1, 1)):
        flag, accepted = _gate_np(*gate, mode)
        assert st[tag] == "0"
        assert np.array_equal(np.fromfile(os.path.join(d, tag + "_accepted.bin"), dtype=np.uint8), accepted)
        assert np.array_equal(np.fromfile(os.path.join(d, tag + "_flag_out.bin"), dtype=np.float32), flag)
    # the restatement itself takes the paths the cases are there for
    flag, accepted = _gate_np(*gate0, 0)
    assert list(accepted) == [0, 0, 1, 1, 1, 0] and flag[(0 * H + 1) * W + 1] == 3.0 and flag[(1 * H + 2) * W + 0] == 0.0
    assert flag[(0 * H + 1) * W + 3] == 2.0 and flag[(0 * H + 0) * W + 2] == 1.0      # the clamped point; one voxel twice in a strand
    flag, accepted = _gate_np(*gate1, 1)
    assert list(accepted) == [0, 1] and flag[(0 * H + 1) * W + 1] == 1.0 and flag[(1 * H + 2) * W + 3] == 1.0
    assert st["acc_none"] == "0"
    assert np.array_equal(np.fromfile(os.path.join(d, "acc_none_flag_out.bin"), dtype=np.float32), gate0[0])


def test_write_sparse_threads_tsan(tmp_path):
    d, st = _build_and_run(tmp_path, "thread", "threads")
    assert st["ws_t1"] == "0" and st["ws_t4"] == "0"
    assert _mat(d, "ws_t1.mat") == _expect(BIG_N, BIG_IDX, BIG_VAL)
    assert _mat(d, "ws_t4.mat") == _mat(d, "ws_t1.mat")
