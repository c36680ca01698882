"""The host rules of the BPR step (gorse_amd/csrc/bpr_plan.hpp: the schedule and the kernel mode of the update launch, chunk and trip
capacity, the preparation route, the flat grid, the scan's form, and the workers, folders and flags of the two update launches) checked
by value in tests/cpp/bpr_plan_main.cpp, which is built and run here under AddressSanitizer and UBSan (no GPU).  Its expected values
were printed from the expressions the launch code held before they moved into the header.  It also holds the accumulated tier's
eligibility (csrc/hot_rows.hpp acc_rows_eligible) to the schedule rule: a handle that gets the tier takes user runs natively."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gorse_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None and shutil.which("clang++") is None, reason="no host C++ compiler")
def test_plan_rules_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    exe = str(tmp_path / "bpr_plan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "bpr_plan_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bpr_plan ok" in out.stdout


def test_the_rules_are_written_once():
    """The user-run gate (its user count and its width list) is hot_rows.hpp's alone, the schedule predicate bpr_plan.hpp's alone, and
    no BPR unit holds a copy of a grid expression the plan states."""
    def source(name):
        with open(os.path.join(CSRC, name)) as f:
            return f.read()

    units = {n: source(n) for n in ("bpr.hip", "bpr_prepare.hip", "bpr_update.hip", "bpr_update_users.hip", "bpr_internal.hpp", "bpr_fold.hpp")}
    plan, hot = source("bpr_plan.hpp"), source("hot_rows.hpp")
    assert "#include <hip" not in plan and "common.hpp" not in plan and "mf_internal.hpp" not in plan
    widths = "d == 8 || d == 16 || d == 32 || d == 64 || d == 128"
    assert hot.count(widths) == 1 and hot.count("constexpr int64_t kUserRunUsers = 4096;") == 1
    assert widths not in plan and "4096" not in re.sub(r"//.*", "", plan)
    assert len(re.findall(r"user_run_width\(d\) && \(U >= kUserRunUsers \|\| forced\)", plan)) == 1
    for name, text in units.items():
        code = re.sub(r"//.*", "", text)
        assert "user_run_width" not in code and "kUserRunUsers" not in code and "4096" not in code and widths not in code, name
        assert "MODE_STORES ? MODE_ATOMIC" not in code and "std::min<int64_t>(ceil_div(" not in code, name
        assert not re.search(r"\b256 \* (8|16)\b", code.replace("std::min<int64_t>(h->U, 256 * 16)", "")), name  # (the grouping pass's own grid)
    # every A/B macro has one definition, in the one unit (or the device header of the one unit) whose code it changes
    assert sum(text.count("#define GORSE_BPR_") for text in units.values()) == 4
