"""The lead-leaf byte model (pgpu_lead_model, pgpu_lead_switch in include/pinot_gpu.h; plan_segment plans with the
same function): bytes per 2048-doc tile of a top-level AND in query order against leading with the top P planes of a
later, more selective child.  CPU only: the arithmetic of DESIGN.md section 4.1 "Lead leaf" on config 5's numbers and
on the shapes that must keep their plan."""
import pytest

from pinot_amd import _lib
from pinot_amd._lib import PGPU_LEAD_RESID_B, PGPU_LEAD_RESID_NONE, PGPU_LEAD_RESID_OTHER, lead_model

MIB = 1 << 20
CARD = 1 << 20      # accountId: 2^20 ids, 20 bits
DAYS = 8 / 1024     # daysSinceEpoch: 8 of 1024 days, 10 bits


def _config5(runs, sel=None, kind=PGPU_LEAD_RESID_B):
    n = sum(hi - lo for lo, hi in runs)
    return lead_model(10, DAYS, kind, 1, 20, n / CARD if sel is None else sel, runs)


def test_config5_leads_with_ten_account_planes():
    m = _config5([(123456, 123457)])
    # today: 10 day planes + 3 prefix planes + 16 candidates x 1/8 covered x 128 B
    assert m.today_bytes == 2560 + 768 + 256 == 3584
    # lead: 10 account planes + 2048 / 1024 survivors x 128 B (+ the day gather of 2048 / 2^20 exact matches)
    assert m.planes == 10
    assert m.lead_bytes == pytest.approx(2560 + 256 + 2048 * 128 / CARD)
    assert round(m.lead_bytes) == 2816
    assert m.num_ranges == 1 and tuple(m.ranges[0]) == (123456 >> 10, (123456 >> 10) + 1)
    # the other widths of the issue's table
    for p, want in ((8, 3072), (12, 3136)):
        assert 256 * p + 2048 * 2.0 ** -p * 128 == want
        assert want > 2816


def test_one_percent_range_keeps_query_order():
    lo = CARD // 3
    m = _config5([(lo, lo + CARD // 100)])
    # every doc in the range gathers the day leaf: 2048 x 1 % x 128 B on top of the planes
    assert m.planes in (8, 10, 12, 16)
    assert m.lead_bytes > 256 * m.planes + 2048 * 0.01 * 128 - 1
    assert m.lead_bytes > m.today_bytes
    assert not _lib.load().pgpu_lead_switch(1e6 * (m.today_bytes - m.lead_bytes), 0)


def test_ids_in_too_many_prefix_ranges_have_no_lead():
    # 5 ids whose top 8 bits all differ and are not neighbours: 5 ranges at every width > PGPU_SLICE_RANGES = 4
    runs = [(k << 16, (k << 16) + 1) for k in (1, 3, 5, 7, 9)]
    m = _config5(runs)
    assert m.planes == 0 and m.lead_bytes == 0
    # today's figure is still the query-order plan's (5 of the 8 three-bit prefixes covered: the prefix planes would
    # cost what they save, so 16 candidates gather a line each)
    assert m.today_bytes == 2560 + 16 * 128
    # four of them are 4 ranges and lead: 12 planes + 2048 x 4 / 4096 x 128 B is the cheapest width
    four = _config5(runs[:4])
    assert four.planes == 12 and four.num_ranges == 4 and four.lead_bytes == pytest.approx(3072 + 256 + 1)
    # neighbours merge: ids in adjacent 8-bit prefixes are one range at P = 8, five ranges at every wider P
    adj = lead_model(10, DAYS, PGPU_LEAD_RESID_B, 1, 20, 5 / CARD, [((k << 12) + 7, (k << 12) + 8) for k in range(5)])
    assert adj.planes == 8 and adj.num_ranges == 1 and tuple(adj.ranges[0]) == (0, 5)


@pytest.mark.parametrize("bits", [6, 9, 11])
def test_narrow_leaf_leads_exactly(bits):
    card = (1 << bits) - 1
    m = lead_model(10, DAYS, PGPU_LEAD_RESID_B, 1, bits, 1 / card, [(card // 2, card // 2 + 1)])
    assert m.planes == bits
    # exact lead leaf: no second gather of its own column
    assert m.lead_bytes == pytest.approx(256 * bits + 2048 / card * 128)
    assert tuple(m.ranges[0]) == (card // 2, card // 2 + 1)


def test_sixteen_bit_leaf_may_lead_with_fewer_planes():
    # P = bits is allowed up to 16 bits, not forced: 10 planes + 2 survivors' lines beat 16 planes
    m = lead_model(10, DAYS, PGPU_LEAD_RESID_B, 1, 16, 2.0 ** -16, [(5, 6)])
    assert m.planes == 10 and m.lead_bytes == pytest.approx(2560 + 256 + 2048 * 2.0 ** -16 * 128)


def test_wider_leaf_never_leads_with_all_its_planes():
    m = lead_model(10, DAYS, PGPU_LEAD_RESID_B, 1, 17, 2.0 ** -17, [(5, 6)])
    assert m.planes in (8, 10, 12, 16) and m.planes < 17


def test_residual_kinds_of_today():
    run = [(77, 78)]
    assert lead_model(10, DAYS, PGPU_LEAD_RESID_NONE, 1, 20, 1 / CARD, run).today_bytes == 2560
    assert lead_model(10, DAYS, PGPU_LEAD_RESID_OTHER, 1, 20, 1 / CARD, run).today_bytes == 2560 + 16 * 128
    # two former dense children are both gathered for the lead leaf's matches
    a = lead_model(20, DAYS, PGPU_LEAD_RESID_B, 1, 20, 0.001, [(0, 1049)])
    b = lead_model(20, DAYS, PGPU_LEAD_RESID_B, 2, 20, 0.001, [(0, 1049)])
    assert b.lead_bytes - a.lead_bytes == pytest.approx(2048 * 0.001 * 128)


def test_threshold_flips_the_decision(monkeypatch):
    lib = _lib.load()
    monkeypatch.delenv("PGPU_LEAD_SWITCH_BYTES", raising=False)
    thr = lib.pgpu_lead_switch_bytes()
    assert thr == 32 * MIB
    m = _config5([(123456, 123457)])
    per_tile = m.today_bytes - m.lead_bytes
    tiles = int(thr // per_tile)
    assert not lib.pgpu_lead_switch(tiles * per_tile, thr)        # just under
    assert lib.pgpu_lead_switch((tiles + 1) * per_tile, thr)      # just over
    assert lib.pgpu_lead_switch(float(thr), thr)
    # config 5 itself (30 x 2^25 docs) is far above it, the test shapes (about 600 tiles) far below
    assert lib.pgpu_lead_switch(30 * (1 << 25) / 2048 * per_tile, thr)
    assert not lib.pgpu_lead_switch(600 * per_tile, thr)
    # 0: whenever cheaper; negative: never
    assert lib.pgpu_lead_switch(1.0, 0) and not lib.pgpu_lead_switch(0.0, 0) and not lib.pgpu_lead_switch(-5.0, 0)
    assert not lib.pgpu_lead_switch(1e12, -1)
    # the knob is read on every call
    # ... and a value that is no integer keeps the default instead of reading as 0
    for v, want in (("0", 0), ("-1", -1), ("4096", 4096), ("off", thr), ("12MiB", thr), ("", thr)):
        monkeypatch.setenv("PGPU_LEAD_SWITCH_BYTES", v)
        assert lib.pgpu_lead_switch_bytes() == want


def test_bad_arguments_are_errors():
    with pytest.raises(_lib.PinotGpuError):
        lead_model(10, DAYS, PGPU_LEAD_RESID_B, 1, 32, 0.5, [(0, 1)])
    with pytest.raises(_lib.PinotGpuError):
        lead_model(10, DAYS, 7, 1, 20, 0.5, [(0, 1)])
    with pytest.raises(_lib.PinotGpuError):
        lead_model(10, DAYS, PGPU_LEAD_RESID_B, 1, 10, 0.5, [(0, 2000)])
