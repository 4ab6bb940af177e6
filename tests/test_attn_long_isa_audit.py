"""Register spills of the key-blocked 16-bit attention kernel (csrc/attention_long.h::attn_long_kernel), read from the built code objects as
tests/test_bc_isa_audit.py reads the policy kernel: both instances the launcher can reach (binary16, bf16), in every unit that launches them, must keep
their registers out of scratch."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def test_long_attention_kernels_do_not_spill():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no ROCm LLVM tools")
    import isa_audit
    seen = set()
    for unit in ("arp_enc.o", "arp_clip.o"):   # the encoder's launches, and arp_op_attention_forms'
        obj = os.path.join(ROOT, "arp_amd", "csrc", unit)
        if not os.path.exists(obj):
            pytest.skip("objects not built")
        rows = isa_audit.audit(obj)
        names = isa_audit.demangle(sorted({r[1] for r in rows}))
        spills = {names[r[1]]: r[3] for r in rows if "attn_long_kernel<" in names[r[1]]}
        assert len(spills) == 2, (unit, sorted(spills))   # <_Float16> and <unsigned short>
        assert all(v == 0 for v in spills.values()), (unit, spills)
        seen |= set(spills)
    assert len(seen) == 2, seen
