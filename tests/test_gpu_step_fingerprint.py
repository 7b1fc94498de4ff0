"""The training step launches what the recorded step launched and leaves the same bits: tools/step_fingerprint.py's cases,
run again on a real MI355X, against tests/golden/step_fingerprint.json.

For EVERY case the trace -- the entry point and stream role of each launch, each `wait_stream`, the GEMM / recurrence /
tail logs -- equals the recorded one; for every case not listed under "unstable" in that file so does the sha256 of every
output and gradient tensor.  This is the check a host-side refactor (functional.py, hip_ops.py, the trainer) is held to.
A change that moves launches or kernels ON PURPOSE records again (`python tools/step_fingerprint.py --record
tests/golden/step_fingerprint.json` on the GPU) and says so.

`test_the_fingerprint_sees_a_moved_launch` shows the record is not blind: with runtime.overlap_wgrad off the sinks case
of one layer launches differently (nothing goes to the side stream, nothing is accumulated by the kernels), and autograd's
two additions leave exactly twice the autograd-return case's gradients."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(os.path.join(ROOT, "tools"))
import step_fingerprint as SF  # noqa: E402
from tssep_amd.train import runtime  # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "step_fingerprint.json")) as f:
    RECORD = json.load(f)


def test_the_record_covers_every_case():
    assert sorted(RECORD["cases"]) == sorted(SF.CASES)
    assert all(name.startswith("D/") for name in RECORD["unstable"]), RECORD["unstable"]
    assert all(("tensors" in c) == (name not in RECORD["unstable"]) for name, c in RECORD["cases"].items())


@pytest.mark.parametrize("name", list(SF.CASES))
def test_step_matches_the_recorded_fingerprint(name):
    want = RECORD["cases"][name]
    trace, tensors = SF.run_case(name)
    assert trace["launches"] == want["launches"], name
    assert trace["trace"] == want["trace"], (name, "same launches, other GEMM / recurrence / tail logs")
    if name not in RECORD["unstable"]:
        got = SF.hashes(tensors)
        assert got == want["tensors"], (name, [k for k in got if got[k] != want["tensors"].get(k)])


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_the_fingerprint_sees_a_moved_launch(prec):
    """tests/test_gpu_rnnp_layer.py::test_sinks_accumulate_twice_the_autograd_gradient states the 2 x; here it is exact."""
    name = f"A/align/act1/{prec}/sinks"
    with runtime.applied(overlap_wgrad=False):
        trace, tensors = SF.run_case(name)
    want = RECORD["cases"][name]
    assert trace["launches"] != want["launches"] and trace["trace"] != want["trace"]
    assert not any("@other" in e for e in trace["launches"]) and any("@other" in e for e in want["launches"])
    _, plain = SF.run_case(f"A/align/act1/{prec}/autograd")
    for k, t in tensors.items():
        assert SF.sha(t) == SF.sha(plain[k] if k == "y" else 2 * plain[k]), k
