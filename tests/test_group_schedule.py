"""The group pipeline's stream / event order (hesaff_amd/csrc/group_schedule.h) on the CPU: the template pipeline.hip runs, over a
recording device, checked by a stand-alone program under AddressSanitizer + UBSan (tests/native/schedule_check.cpp) - the hazards the
order exists for at every group count 0 .. 10 under every option, that each wait and record is needed, and equality with the
sequences of the code the header replaced (tests/golden/group_schedule_parent.txt)."""
from tests.schedule_native import run_schedule_check


def test_group_schedule(tmp_path):
    run_schedule_check(tmp_path, "upright")
