"""A checkout that was built and then made read-only: the library loads without the build lock, and bench.py puts the stand-in
checkpoints in a per-user cache instead of <repo>/weights — the same weights as the in-tree ones."""
import os
import sys
from pathlib import Path
from types import SimpleNamespace

import torch

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def test_up_to_date_library_loads_without_the_build_lock(monkeypatch):
    from omniparser_amd import build as B
    B.build_lib(verbose=False)                       # no-op after build()

    class Refused:
        def __enter__(self):
            raise PermissionError("read-only checkout")

        def __exit__(self, *exc):
            return False
    monkeypatch.setattr(B, "_BuildLock", Refused)
    assert B.ensure_built() == B.LIB


def test_bench_checkpoints_go_to_the_user_cache_when_the_tree_is_read_only(monkeypatch, tmp_path):
    import bench
    from tools.make_weights import ensure_blob
    in_tree = ensure_blob(seed=0, nc=1, width=0.25)
    ro = tmp_path / "checkout"                       # an empty checkout, not writable
    ro.mkdir()
    real_access = os.access

    def access(path, mode):
        p = str(path)
        return False if (mode & os.W_OK) and (p == str(ro) or p.startswith(str(ro) + os.sep)) else real_access(path, mode)
    monkeypatch.setattr(bench.os, "access", access)
    monkeypatch.setattr(bench, "ROOT", ro)
    monkeypatch.setenv("XDG_CACHE_HOME", str(tmp_path / "cache"))
    monkeypatch.setenv("OMNI_WEIGHTS_DIR", "")           # restored (unset) after the test: bench.py sets it
    blob, cap = bench.standin_checkpoints(SimpleNamespace(mode="detect", width=0.25), 0, 1)
    wdir = tmp_path / "cache" / "omniparser_amd" / "weights"
    assert os.environ["OMNI_WEIGHTS_DIR"] == str(wdir)
    assert blob == wdir / Path(*in_tree.parts[-3:]) and blob.exists() and cap.parent == wdir
    assert not (ro / "weights").exists()
    a, b = torch.jit.load(str(blob)).state_dict(), torch.jit.load(str(in_tree)).state_dict()
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    # a second run finds them there and generates nothing
    mtime = blob.stat().st_mtime_ns
    assert bench.standin_checkpoints(SimpleNamespace(mode="detect", width=0.25), 0, 1)[0] == blob and blob.stat().st_mtime_ns == mtime
