"""CPU-only: the per-view scratch sizes of the strand tools (mh_capture_scratch_bytes, mh_photo_scratch_bytes,
mh_support_scratch_bytes) equal the closed forms of include/mh_pmvo.h.  The guard tests place their canaries directly
behind these sizes, so a layout that grows or shrinks must show here, without a GPU: the queries launch nothing.  The
comparison itself is tests/scratch_sizes_main.cpp, a stand-alone host program that loads the built library."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scratch_sizes_equal_the_closed_forms(tmp_path):
    from monohair_amd import _lib

    assert os.path.exists(_lib.LIB_PATH), "build with __graft_entry__.build()"
    cxx = os.environ.get("CXX") or shutil.which("g++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "scratch_sizes_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "scratch_sizes_main.cpp"), "-ldl"])
    r = subprocess.run([exe, _lib.LIB_PATH], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, "exit status %d\n%s" % (r.returncode, r.stderr[-4000:])
    assert len(r.stdout.splitlines()) == 7 * 3 * 4       # every size of the grid was asked for
