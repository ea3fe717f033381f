"""Section `gpu` of tests/golden/gemm_asm_plans.json (tests/test_gemm_asm_plans_host.py describes the file): launches of more tiles
than the device has compute units, where ll_gemm_plan_epi names the persistent kernels gemm_asmp_* / gemm_asmp_*_m16, and the split-K
plan of the small-M shapes.  Plans only: no kernel is launched."""
import json

import pytest

import test_gemm_asm_plans_host as H

pytestmark = pytest.mark.gpu


def test_gpu_plans_equal_the_recording():
    lib = H._lib()
    recorded, cus = json.load(open(H.GOLDEN))["gpu"]["cus"], H.device_cus(lib)
    assert cus == recorded, (f"this device has {cus} compute units, the recording was made on one with {recorded}: the persistent plans "
                             "and the split-K plan depend on the count, so the recording does not describe this device")
    bad = H.mismatches(lib, "gpu")
    assert not bad, f"{len(bad)} answers differ from the recording, the first: " + "; ".join(bad[:5])
