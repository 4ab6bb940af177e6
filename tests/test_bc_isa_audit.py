"""Register spills of the BC form of the fused policy kernel (policy_fused_bc_kernel, two tokens per time step), read from the built code object as
tests/test_isa_audit.py reads the ARP-DT instance: every instance the step can launch must keep its registers out of scratch."""
import glob
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def test_bc_policy_kernel_does_not_spill():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no ROCm LLVM tools")
    import isa_audit
    obj = os.path.join(ROOT, "arp_amd", "csrc", "arp_dt.o")
    if not os.path.exists(obj):
        pytest.skip("objects not built")
    rows = isa_audit.audit(obj)
    names = isa_audit.demangle(sorted({r[1] for r in rows}))
    spills = {names[r[1]]: r[3] for r in rows if "policy_fused_bc_kernel<" in names[r[1]]}
    for inst in ("<128, 512, true>", "<128, 512, false>", "<64, 256, true>", "<64, 256, false>"):
        assert any(inst in k for k in spills), (inst, sorted(spills))
    assert all(v == 0 for v in spills.values()), spills
    assert not glob.glob(os.path.join(ROOT, "arp_amd", "csrc", "*.o.0.*"))
