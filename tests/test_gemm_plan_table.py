"""The GEMM dispatcher decides what it decided when tests/golden/gemm_plan.json was recorded (host only, no GPU):
tools/gemm_plan_table.py's corpus -- > 10 000 row x row and > 2 000 weight-gradient requests -- through tssep_gemm_plan
under `auto` and on every kernel by name, tssep_gemm_wgrad_splits and tssep_gemm_wgrad_split_rule, every entry equal.

This is the check a refactor of the dispatcher (csrc/gemm_rules.h, the candidate table of csrc/gemm_bf16x3.hip) is held
to.  A change that alters a rule ON PURPOSE records again (`python tools/gemm_plan_table.py --record
tests/golden/gemm_plan.json`) and says so."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(os.path.join(ROOT, "tools"))
import gemm_plan_table as PT  # noqa: E402

RECORD = os.path.join(ROOT, "tests", "golden", "gemm_plan.json")


def test_the_record_covers_every_kernel_within_the_size_cap():
    with open(RECORD) as f:
        want = json.load(f)
    assert want["requests"] - want["weight_gradients"] >= 10000 and want["weight_gradients"] >= 2000
    assert len(want["index"]) == 2 * want["requests"]
    assert {r[0] for r in want["records"]} >= set(PT.CHOICE[1:]), "every kernel id is some request's automatic choice"
    assert os.path.getsize(RECORD) <= 200 * 1000


def test_the_dispatcher_matches_the_recorded_plan_table(capsys):
    rc = PT.main(["--check", RECORD])
    assert rc == 0, capsys.readouterr().out
