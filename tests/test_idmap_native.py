"""Host-sanitizer run of the stable-id calls of the C ABI:
tests/native/idmap_check.cpp linked against the host C++ (fx_index.cpp, fx_api_*.cpp, fx_plan.cpp) built with
-fsanitize=address,undefined on the host side (`make -C
rag-faiss-embedding_amd/csrc asan`, also run by __graft_entry__.build()), the
way tests/test_native_asan.py runs abi_check.  The driver walks
fx_index_add_with_ids (ragged growth, host and device ids), fx_index_has_ids,
fx_index_get_ids, fx_index_rows_of_ids, the mode rules, a search, a selector
and a removal by label, and the IxM2 write / read with every truncation of the
file, checked against a brute force on the host.  Any ASan / UBSan report
fails the run."""
import os
import subprocess
from pathlib import Path

import pytest

BIN = Path(__file__).resolve().parent / "native" / "_build" / "idmap_check"


@pytest.mark.gpu
def test_idmap_abi_under_host_sanitizers(tmp_path):
    assert BIN.exists(), f"{BIN} not built: make -C rag-faiss-embedding_amd/csrc asan"
    env = dict(os.environ, TMPDIR=str(tmp_path),
               # the HIP runtime's own allocations are not ours to leak-check
               ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(BIN)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"rc={r.returncode}\n{r.stdout[-4000:]}\n{r.stderr[-8000:]}"
    assert "idmap_check ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-8000:]
