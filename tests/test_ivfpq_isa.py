"""Static ISA check of the gather list scan (CPU only): fx_ivfpq.hip compiled to gfx950 assembly must
show no LDS-DMA hazard under tools/check_dma_hazards.py (tests/test_isa_hazards.py explains the two
hazards), and k_ivfpq_scan must run without private (scratch) memory: its stage waits are
`s_waitcnt vmcnt(0)` on the LDS-DMA in flight, and a spill would put scratch
traffic into the tile loop."""
import re
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "rag-faiss-embedding_amd" / "csrc"
HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not available")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa_ivfpq")
    s = out / "fx_ivfpq.s"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                        str(CSRC / "fx_ivfpq.hip"), "-o", str(s)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    yield s
    shutil.rmtree(out, ignore_errors=True)


def test_no_dma_hazards(asm):
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "check_dma_hazards.py"), str(asm)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "0 hazard(s)" in r.stdout


def test_list_scan_uses_no_scratch_and_the_bf16_mfma(asm):
    text = asm.read_text()
    sizes = re.findall(r"\.name:\s+(_ZN2fx\S*k_ivfpq_scan\S+)\s+\.private_segment_fixed_size:\s+(\d+)", text)
    assert len(sizes) == 2, f"two k_ivfpq_scan instances (L2, IP) were expected: {sizes}"
    bad = [(n, int(v)) for n, v in sizes if int(v) != 0]
    assert not bad, f"k_ivfpq_scan with scratch: {bad}"
    for m in re.finditer(r"^(_ZN2fx\w*?k_ivfpq_scan\w+):", text, re.M):
        body = text[m.end():text.find(".Lfunc_end", m.end())]
        assert body.count("v_mfma_f32_16x16x32_bf16") >= 48, m.group(1)  # 3 products x 4 x 4 per stage
        assert "global_load_lds_dwordx4" in body, m.group(1)
