"""CPU: the designed inputs of the edge variants (tests/edgevar_cases.py) are what they claim to be -- the helper's ops expand back to the
hand-written strings, and the cases have the properties the kernels are to be tried on."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import edgevar_cases as EC  # noqa: E402
from isocon_amd import SW_alignment_module as SWM  # noqa: E402

CASES = {cs["name"]: cs for cs in EC.designed_cases()}


def test_ops_expand_to_the_strings():
    for cs in list(CASES.values()) + EC.g16_cases():
        ops_tc, ops_ct = EC.ops_of_case(cs)
        assert SWM._ops_to_alignment(ops_tc, cs["t"], cs["c"]) == cs["tc"], cs["name"]
        assert SWM._ops_to_alignment(ops_ct, cs["c"], cs["t"]) == cs["ct"], cs["name"]
        assert all(op >> 4 > 0 and op & 15 < 4 for op in ops_tc + ops_ct)
    assert EC.mirrored(EC.ops_of_rows("AC-GT", "A-TGA")) == EC.ops_of_rows("A-TGA", "AC-GT")
    assert len(EC.g16_cases()) == 70


def records(name):
    return EC.expected_records(CASES[name])[1]


def test_masked_ends_and_no_variants():
    for name in ("identical", "end_gaps_t_leads_c_trails", "end_gaps_c_leads_t_trails"):
        assert EC.expected_tuple(CASES[name]) == ([], {}, {}, {}, {}), name
    assert CASES["end_gaps_t_leads_c_trails"]["tc"][0].startswith("-") and CASES["end_gaps_t_leads_c_trails"]["tc"][1].endswith("-")
    assert CASES["end_gaps_c_leads_t_trails"]["tc"][1].startswith("-") and CASES["end_gaps_c_leads_t_trails"]["tc"][0].endswith("-")
    assert [r[0] for r in records("variant_next_to_masked_runs")] == [2, 9]          # masked: columns 0, 1 and 10, 11
    assert [(r[0], r[6]) for r in records("deletion_right_after_masked_run")] == [(2, "D")]
    assert [(r[0], r[6]) for r in records("insertion_right_before_masked_run")] == [(8, "I")]


def test_columns_and_row_lengths():
    assert [r[0] for r in records("s_at_0_63_64_65_last")] == [0, 63, 64, 65, 129]
    assert records("s_at_0_63_64_65_last")[0][9:] == tuple(row[0:2] for row in reversed(CASES["s_at_0_63_64_65_last"]["tc"]))          # max(0, i - 1)
    assert len(records("s_at_0_63_64_65_last")[-1][9]) == 2          # cut at the row's end
    assert {len(CASES[n]["tc"][0]) for n in ("row_1", "row_63", "row_64", "row_65", "row_129")} == {1, 63, 64, 65, 129}
    assert records("row_1") == [(0, 0, 0, 0, 0, 1, "S", "A", "C", "C", "A")]
    assert len(records("snippet_past_end")[0][9]) < records("snippet_past_end")[0][5] + 2


def test_homopolymers():
    assert {n: records(n)[0][5] for n in CASES if n.startswith("d_run") and n[5].isdigit()} == {
        "d_run1_base0": 1, "d_run2_base0": 2, "d_run2_base1": 2, "d_run5_base0": 5, "d_run5_base2": 5, "d_run5_base4": 5}
    assert records("d_run_touches_first_base")[0][1:6] == (1, 0, 1, 1, 3) and records("d_run_touches_last_base")[0][1:6] == (6, 5, 6, 6, 3)
    r = records("d_run_straddles_64")[0]
    assert (r[0], r[1], r[5], r[6]) == (64, 64, 5, "D")
    assert {n: records(n)[0][5:7] for n in CASES if n.startswith("i_equals")} == {
        "i_equals_left_run": (2, "I"), "i_equals_right_run": (2, "I"), "i_equals_both_runs": (5, "I"), "i_equals_neither": (1, "I")}
    assert records("i_equals_left_run")[0][1] + 1 == records("i_equals_right_run")[0][1] + 2          # (the gap sits behind / in front of t's A)


def test_shared_keys_overwrite():
    two = records("two_base_insertion")
    assert [r[3] for r in two] == [3, 3] and [r[4] for r in two] == [3, 4]
    got = EC.expected_tuple(CASES["two_base_insertion"])
    assert list(got[1].items()) == [(3, ("I", "A", 1))] and len(got[2]) == 2          # the later variant wins on t
    two = records("two_base_deletion_in_run")
    assert [r[3] for r in two] == [3, 4] and [r[4] for r in two] == [3, 3] and len(EC.expected_tuple(CASES["two_base_deletion_in_run"])[2]) == 1


def test_many_ops_capacity_and_orientation():
    assert len(EC.ops_of_case(CASES["ops_70"])[0]) == 70 and len(EC.ops_of_case(CASES["ops_140"])[0]) == 140
    ops_tc, ops_ct = EC.ops_of_case(CASES["exon_400"])
    assert ops_tc == [30 << 4, 400 << 4 | 2, 30 << 4] and EC.capacity(ops_tc, ops_ct) == 400 == len(records("exon_400"))
    flips = {n: (EC.expected_records(CASES[n])[0], len(EC.expected_records(CASES[n])[1])) for n in ("ct_has_fewer", "ct_has_as_many", "ct_has_more")}
    assert flips == {"ct_has_fewer": (True, 1), "ct_has_as_many": (False, 1), "ct_has_more": (False, 1)}
    assert records("ct_has_as_many")[0][0] == 4          # (the (c, t) list would have put it in column 3)


def test_refused_lists():
    names = [r[0] for r in EC.refused_ops()]
    assert names[:6] == ["one_long_of_t", "one_short_of_t", "one_long_of_c", "one_short_of_c", "code_4", "code_4_in_second_list"]
    for name, t, c, ops_tc, ops_ct in EC.refused_ops():
        used_t = sum(op >> 4 for op in ops_tc if op & 15 in (0, 1, 2))
        used_c = sum(op >> 4 for op in ops_tc if op & 15 in (0, 1, 3))
        if name.startswith("one_"):
            assert (used_t - len(t), used_c - len(c)) == {"one_long_of_t": (1, 0), "one_short_of_t": (-1, 0), "one_long_of_c": (0, 1), "one_short_of_c": (0, -1)}[name]
