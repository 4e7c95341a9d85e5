"""The recorded table of the light traces' return codes (tests/golden/light_errors.json) covers every light entry
point the package binds, with the case count tests/lighterrors.py generates for each."""
import sphereflake_amd as sf
import lighterrors as le


def test_golden_lists_every_light_entry_with_its_case_count():
    table = le.load_golden()
    light = {n for n in sf.SIGNATURES if n.startswith("sf_trace_")} - {"sf_trace_dirs_to", "sf_trace_dirs",
                                                                        "sf_trace_rays_to"}
    assert set(table) == light == {e[0] for e in le.ENTRIES}
    for entry in le.ENTRIES:
        k = len(le.faults_of(entry))
        codes = table[entry[0]]
        assert len(codes) == len(le.cases_of(entry)) == 1 + k + k * (k - 1) // 2, entry[0]
        assert set(codes) <= set("0123456789") and codes[0] == "0", entry[0]   # (the fault-free call succeeds)
        assert codes[1] == "5", entry[0]   # (the first fault is `noview`: SF_ENOVIEW)
