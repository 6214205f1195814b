"""oracle.build() under concurrent use: processes that find the checker stale at the same time (the two ranks of tests/test_dist_gloo.py
after the source changed) must all load a complete library.  Runs on a copy of oracle/ so that the tree's own build is left alone."""
import os
import shutil
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_processes_that_find_the_oracle_stale_together_all_load_it(tmp_path):
    work = tmp_path / "oracle"
    work.mkdir()
    for name in ("__init__.py", "oracle.py", "locohd_oracle.c", "Makefile"):
        shutil.copy(ROOT / "oracle" / name, work / name)
    code = (f"import sys; sys.path.insert(0, {str(tmp_path)!r}); from oracle import oracle as o; "
            "print(o.WeightFunction('uniform', [3.0, 10.0]).integral_point(6.5))")
    env = {k: v for k, v in os.environ.items() if k != "LCHD_ASAN"}
    for _ in range(2):  # no library yet; then a library older than its source
        procs = [subprocess.Popen([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env) for _ in range(4)]
        for p in procs:
            out, err = p.communicate(timeout=120)
            assert p.returncode == 0 and out.strip() == b"0.5", err[-600:].decode(errors="replace")
        so = work / "liblocohd_oracle.so"
        os.utime(work / "locohd_oracle.c", (so.stat().st_mtime + 10, so.stat().st_mtime + 10))
    assert [p.name for p in work.glob("tmp*")] == []  # every library linked under a name of its own was renamed into place
