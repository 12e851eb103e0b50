"""gfx950 VALU cross-lane helpers of the scan and the refine (fx_device.h
lane_xor<S>: DPP quad_perm / row_ror inside 16-lane rows, v_permlane16_swap
and v_permlane32_swap across them; the bitonic sort64 built on them): checked
on the device against their definition, through a small probe kernel compiled
with the same headers (hipcc, gfx950)."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "rag-faiss-embedding_amd" / "csrc"
PROBE = ROOT / "tests" / "native" / "lane_probe.hip"
LIB = ROOT / "tests" / "native" / "_build" / "liblane_probe.so"


def build_probe():
    LIB.parent.mkdir(parents=True, exist_ok=True)
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                    f"-I{CSRC}", "-o", str(LIB), str(PROBE)], check=True)


def test_probe_builds():
    """CPU: the probe compiles for gfx950 (the driver's GPU run loads it)."""
    build_probe()
    assert LIB.exists()


@pytest.mark.gpu
def test_lane_swaps_on_device():
    import torch  # noqa: F401  (one HIP runtime per process)
    if not LIB.exists():
        pytest.fail(f"{LIB} missing: build it first (__graft_entry__.build(), or on the CPU "
                    "tests/test_lane_swap.py::test_probe_builds)")
    lib = ctypes.CDLL(str(LIB))
    rng = np.random.default_rng(4)
    keys = rng.integers(0, 9, 64).astype(np.float32)           # many duplicate keys: ties -> smaller id
    keys[rng.integers(0, 64, 5)] = np.inf
    out = np.zeros((9, 64), dtype=np.int32)
    kout = np.zeros(64, dtype=np.float32)
    rc = lib.lane_probe(keys.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p),
                        kout.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    x = (np.arange(64) * 7 + 3) % 11
    lane = np.arange(64)
    for row, s in enumerate((1, 2, 4, 8, 16, 32)):
        assert (out[row] == x[lane ^ s]).all(), (s, out[row])
    assert (out[6] == x[lane ^ 48]).all(), out[6]
    assert (out[7] == x[lane ^ 7]).all(), out[7]
    ids = (lane * 37) % 64
    order = sorted(range(64), key=lambda j: (keys[j], ids[j]))
    assert (kout == keys[order]).all() and (out[8] == ids[order]).all()
