"""The return codes of the light traces under one fault, under every pair of faults and under none equal the recorded
table tests/golden/light_errors.json (tests/lighterrors.py: the cases, and how the table was recorded)."""
import pytest

import sphereflake_amd as sf
import lighterrors as le

pytestmark = pytest.mark.gpu


def test_return_codes_equal_the_recorded_table():
    sf.build()
    assert sf.device_count() >= 1, "no HIP device visible: GPU tests must run on an MI355X"
    got, want = le.run(), le.load_golden()
    assert set(got) == set(want)
    where = le.first_difference(got, want)
    assert where is None, "%s with faults %s returns %s, recorded %s" % where
    assert got == want
