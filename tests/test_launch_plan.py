"""The launch geometry of the tuner's kernels and of the spectrum launches (webradio_amd/csrc/wr_plan.h): the arithmetic alone, no GPU.  Every expected
figure is worked by hand from the rule as the launch functions had it before the plans were split out of them (the working
stands beside each), never taken from a run of the code under test."""
import pytest

import launch_plan as lp
from launch_plan import WR_NCO_EXACT, WR_NCO_ROTATE, WR_NCO_SPLIT

D2S = [1, 2, 3, 4, 5, 6, 8, 10]             # the audio decimations the post stage is built for
CU_LDS = 160 * 1024


def test_supported_audio_decimations():
    assert [d for d in range(0, 40) if lp.lib().wr_plan_post_d2_supported(d)] == D2S
    assert lp.post_tk() == 16


# ---- the streaming launch's post tiling --------------------------------------------------------------------------------
# tiles = ceil(k2 / 16); tasks(run) = ceil(tiles / run) * groups.
#   min_run : the least run with tasks <= n_post
#   run     : min_run -- or, if min_run >= 2 and n_post >= 8, the least run with tasks <= n_post / 2 ("long") --
#             then + 1 while run < 4, run < tiles and n_post / 4 < tasks(run) <= n_post / 2 ("loop")
#   drain   : min(min_run, run)
# n_post = 252: n_post / 2 = 126, n_post / 4 = 63.
@pytest.mark.parametrize("k2,groups,n_post,want", [
    # run-1-ragged: 4 tiles x 1 group = 4 tasks <= 252; 4 is not above 63: no loop
    (60, 1, 252, dict(tiles=4, min_run=1, run=1, ntiles=4, drain_run=1, drain_ntiles=4, long_runs=False, widened=0)),
    # run-2: 50 tiles x 2 = 100 <= 252; 63 < 100 <= 126 -> run 2: 25 x 2 = 50, not above 63
    (790, 2, 252, dict(tiles=50, min_run=1, run=2, ntiles=25, drain_run=1, drain_ntiles=50, long_runs=False, widened=1)),
    # run-3: 25 tiles x 5 = 125 <= 252; 63 < 125 <= 126 -> run 2: 13 x 5 = 65, still -> run 3: 9 x 5 = 45
    (393, 5, 252, dict(tiles=25, min_run=1, run=3, ntiles=9, drain_run=1, drain_ntiles=25, long_runs=False, widened=2)),
    # run-4: 300 tiles x 1: 300 > 252, 150 <= 252 -> min_run 2; long: 150 > 126, 100 <= 126 -> 3; 63 < 100 <= 126 -> 4 (the cap)
    (4790, 1, 252, dict(tiles=300, min_run=2, run=4, ntiles=75, drain_run=2, drain_ntiles=150, long_runs=True, widened=1)),
    # long-runs: 225 tiles x 2: 450, 226 <= 252 -> min_run 2; long: 226, 150 > 126, 57 x 2 = 114 <= 126 -> 4; no loop at 4
    (3595, 2, 252, dict(tiles=225, min_run=2, run=4, ntiles=57, drain_run=2, drain_ntiles=113, long_runs=True, widened=0)),
    # one tile: run < tiles never holds
    (9, 3, 252, dict(tiles=1, min_run=1, run=1, ntiles=1, drain_run=1, drain_ntiles=1, long_runs=False, widened=0)),
    (16, 16, 12, dict(tiles=1, min_run=1, run=1, ntiles=1, drain_run=1, drain_ntiles=1, long_runs=False, widened=0)),
    # n_post < 8: the long-run rule must not apply.  20 tiles, n_post = 6: 20, 10, 7 > 6, 5 <= 6 -> min_run 4 (tasks for
    # n_post / 2 = 3 would have been run 7); 10 tiles, n_post = 7: 10 > 7, 5 <= 7 -> 2 (for 3: run 4); 5 is not <= 7 / 2
    (320, 1, 6, dict(tiles=20, min_run=4, run=4, ntiles=5, drain_run=4, drain_ntiles=5, long_runs=False, widened=0)),
    (160, 1, 7, dict(tiles=10, min_run=2, run=2, ntiles=5, drain_run=2, drain_ntiles=5, long_runs=False, widened=0)),
])
def test_stream_post_tiling(k2, groups, n_post, want):
    assert lp.stream_tiling(k2, groups, n_post)._asdict() == want


# ---- the streaming launch's roles: per_cu capped at 3, fewer than 2 none; n_ddc = (per_cu - 1) * CUs, n_post = CUs - 4 ----
@pytest.mark.parametrize("per_cu,num_cus,want", [
    (3, 256, (512, 252)),
    (5, 256, (512, 252)),                   # the cap at three
    (2, 256, (256, 252)),
    (1, 256, (0, 0)),
    (3, 4, (0, 0)), (3, 1, (0, 0)), (3, 0, (0, 0)),     # no post workgroup to give: no launch, and no wrap
    (3, 5, (10, 1)),
])
def test_stream_roles(per_cu, num_cus, want):
    assert lp.stream_roles(per_cu, num_cus) == want


def test_lds_sizes():
    L = lp.lib()
    # post stage at D2 = 5: ((15 * 5 + 64 nseg) rows * 64 + the tile 16 * 65 + 64 modes) floats
    #   nseg 1: (139 * 64 + 1040 + 64) * 4 = 10 000 * 4 = 40 000; the streaming launch adds 16 words: 40 064
    #   nseg 2: (203 * 64 + 1104) * 4 + 64 = 56 448;  nseg 4: (331 * 64 + 1104) * 4 + 64 = 89 216
    assert L.wr_plan_post_lds_bytes(5, 1) == 40_000
    assert [L.wr_plan_stream_lds_bytes(5, 1, nseg) for nseg in (1, 2, 4)] == [40_064, 56_448, 89_216]
    # the DDC's side wins only where the post stage is small: D2 = 1, four window copies: 8 * 2 * 512 * 4 + 2 * 256 * 8 = 36 864
    # against (15 + 64) * 64 + 1104 = 6 160 floats = 24 640 + 64
    assert L.wr_plan_stream_lds_bytes(1, 4, 1) == 36_864
    assert not L.wr_plan_stream_nseg_supported(4, 4) and L.wr_plan_stream_nseg_supported(3, 4)
    assert L.wr_plan_stream_nseg_supported(10, 1) and L.wr_plan_stream_nseg_supported(10, 2)
    assert not L.wr_plan_stream_nseg_supported(1, 3)


def test_stream_plan():
    # one filter, an even number of lane groups: NG = 2; several filters in a lane group: TS = 4 and kmax window copies
    assert lp.stream_plan(5, 4, 1, True, 1) == (True, 2, 1, 40_064)
    assert lp.stream_plan(5, 3, 1, True, 1) == (True, 1, 1, 40_064)
    assert lp.stream_plan(5, 4, 1, False, 2) == (True, 1, 1, 56_448)
    assert lp.stream_plan(1, 4, 3, False, 1) == (True, 1, 4, 8 * 2 * 512 * 3 + 4096)
    for d2, groups, kmax, nseg in [(7, 4, 1, 1), (5, 0, 1, 1), (5, 17, 1, 1), (5, 4, 0, 1), (5, 4, 5, 1), (4, 4, 1, 4), (5, 4, 1, 3)]:
        assert not lp.stream_plan(d2, groups, kmax, True, nseg).ok, (d2, groups, kmax, nseg)


# ---- the group map: entry i (eight bits each, sixteen entries) = the i-th selected lane group ----
def test_group_map():
    assert lp.group_map(4) == (0x03020100, 0, 4, 0, 1, [0, 1, 2, 3])
    assert lp.group_map(4, gsel=0b1010) == (0x0301, 0, 2, 0, 1, [1, 3])
    m = lp.group_map(17)
    assert (m.gmap0, m.gmap1, m.ngroups, m.rest) == (0x0706050403020100, 0x0F0E0D0C0B0A0908, 16, 1 << 16)
    assert m.order == list(range(16))
    m = lp.group_map(64)
    assert (m.gmap0, m.gmap1, m.ngroups, m.rest) == (0x0706050403020100, 0x0F0E0D0C0B0A0908, 16, 0xFFFF_FFFF_FFFF_0000)
    # the groups a launch leaves for the next come out of `rest` in ascending order too
    m = lp.group_map(20, gsel=m.rest)
    assert (m.ngroups, m.rest, m.order) == (4, 0, [16, 17, 18, 19])
    assert lp.group_map(0).ngroups == 0 and lp.group_map(3, gsel=1 << 5).ngroups == 0
    # kmax: over the mapped groups only
    nsets = [1, 3, 2, 4]
    assert lp.group_map(4, nsets=nsets).kmax == 4
    assert lp.group_map(4, gsel=0b0101, nsets=nsets).kmax == 2
    assert lp.group_map(4, gsel=0b0011, nsets=nsets).kmax == 3
    assert lp.group_map(18, gsel=0, nsets=[1] * 16 + [4, 4]).kmax == 1       # groups 16, 17 are not in this launch


@pytest.mark.parametrize("d1,k1,want", [(400, 10_000, 1), (1, 65, 63), (3, 10, 10), (64, 0, 0), (63, 5, 1), (62, 5, 2), (0, 0, 0)])
def test_kslow(d1, k1, want):
    """ceil(63 / d1), k1 at most; a block without an output frame has none (the launch never worked the quotient out for it)"""
    assert lp.lib().wr_plan_kslow(d1, k1) == want


def test_post_tilings_of_a_block():
    # riding: tiles x groups >= 1536: runs of 4, >= 384: 2, else 1
    assert lp.post_tiling_riding(125, 4) == (2, 63)          # C2: 500
    assert lp.post_tiling_riding(125, 3) == (1, 125)         # 375
    assert lp.post_tiling_riding(96, 16) == (4, 24)          # 1536
    assert lp.post_tiling_riding(383, 1) == (1, 383) and lp.post_tiling_riding(384, 1) == (2, 192)
    # on its own: one tile per workgroup up to 4096 tiles x groups; 256 taps: runs of 2 from 384 on
    assert lp.post_tiling_alone(125, 4) == (1, 125)
    assert lp.post_tiling_alone(500, 8) == (1, 500) and lp.post_tiling_alone(513, 8) == (2, 257)     # 4000, 4104
    assert lp.post_tiling_alone(125, 4, nseg=4) == (2, 63) and lp.post_tiling_alone(125, 4, nseg=2) == (1, 125)
    assert lp.post_tiling_alone(95, 4, nseg=4) == (1, 95)    # 380


# ---- the per-block DDC --------------------------------------------------------------------------------------------------
def _headline(**kw):
    """ROTATE, folded taps, the post stage (D2 = 5, k2 = 2 000: 125 tiles) riding, 256 channels on one filter, 256 CUs"""
    groups = kw.pop("groups", 4)
    run, ntiles = lp.post_tiling_riding(125, groups)
    a = dict(nco=WR_NCO_ROTATE, utaps=True, pd2=5, groups=groups, k1=10_000, d1=400, num_cus=256, one_filter=True, min_passes=4,
             post_ntiles=ntiles, post_groups=groups)
    a.update(kw)
    return lp.ddc_plan(**a)


def test_ddc_plan_headline():
    # waves2 = 256 CUs * (6 * 4 / 8 - 1) * 8 = 4 096; 10 000 * (4 / 2) = 20 000 >= 4 * 4 096: NG = 2
    # lds = max(8 * 2 * 512 + 2 * 256 * 8 = 12 288, 40 000); wgs_per_cu = min(6 * 4 / 8 = 3, 163 840 / 40 000 = 4) - 1 = 2
    # riding tiling: 125 x 4 = 500 >= 384: run 2, 63 workgroups + the state one, x 4 groups = 256
    # kslow = ceil(63 / 400) = 1, n_bnd = ceil(1 * 4 / 8) = 1, units = 9 999 * 2; wgs = min(ceil(19 998 / 8) = 2 500, 256 * 2)
    p = _headline()
    assert p == (4, 0, 2, 8, 1, 40_000, 2, 256, 1, 1, 19_998, 512)
    assert p.wgs + p.n_bnd + p.post_wgs == 769


def test_ddc_plan_ng2_threshold():
    # the threshold: k1 * 2 >= 4 * 4 096, k1 >= 8 192
    # 8 191: NG = 1: wgs_per_cu = min(4, 4) - 1 = 3; units = 8 190 * 4 = 32 760, 4 095 workgroups -> 256 * 3
    assert _headline(k1=8_191) == (4, 0, 1, 8, 1, 40_000, 3, 256, 1, 1, 32_760, 768)
    # 8 192: NG = 2: units = 8 191 * 2 = 16 382 -> 2 048 -> 512
    assert _headline(k1=8_192) == (4, 0, 2, 8, 1, 40_000, 2, 256, 1, 1, 16_382, 512)
    # min_passes = 0: always, down to one frame: kslow = 1 = k1, no units; two lane-group pairs still need a wave each: one workgroup
    assert _headline(k1=1, min_passes=0) == (4, 0, 2, 8, 1, 40_000, 2, 256, 1, 1, 0, 1)
    # no post stage riding: waves2 = 256 * 3 * 8 = 6 144, the threshold is 12 288; lds 12 288; three workgroups per CU
    assert _headline(pd2=0, k1=12_287, post_ntiles=0, post_groups=0) == (4, 0, 1, 8, 1, 12_288, 4, 0, 1, 1, 12_286 * 4, 1024)
    assert _headline(pd2=0, k1=12_288, post_ntiles=0, post_groups=0) == (4, 0, 2, 8, 1, 12_288, 3, 0, 1, 1, 12_287 * 2, 768)
    # several channel filters: never
    assert _headline(one_filter=False).ng == 1


def test_ddc_plan_odd_group_count():
    # 3 lane groups: NG = 1; 125 x 3 = 375 < 384: run 1, (125 + 1) x 3 = 378 post workgroups; n_bnd = ceil(3 / 8) = 1
    # units = 9 999 * 3 = 29 997 -> 3 750 workgroups -> 256 * 3
    assert _headline(groups=3) == (3, 0, 1, 8, 1, 40_000, 3, 378, 1, 1, 29_997, 768)


def test_ddc_plan_tap_sets():
    # a lane group that mixes three channel filters: three window copies per buffer: 8 * 2 * 512 * 3 + 4 096 = 28 672
    p = lp.ddc_plan(WR_NCO_ROTATE, True, 0, 4, 1000, 8, 256, one_filter=False, nsets=[1, 3, 1, 2])
    # kslow = ceil(63 / 8) = 8, n_bnd = ceil(8 * 4 / 8) = 4, units = 992 * 4 -> 496 workgroups
    assert p == (4, 0, 1, 8, 3, 28_672, 4, 0, 8, 4, 3_968, 496)


def test_ddc_plan_per_lane_taps():
    # ROTATE, per-lane taps: 8 waves, windows + tables + one lane group's taps: 8 192 + 4 096 + 64 * 64 * 4 = 28 672; no roles
    # 7 lane groups, k1 = 100: 700 units -> 88 workgroups -> a whole number per lane group: 84
    assert lp.ddc_plan(WR_NCO_ROTATE, False, 0, 7, 100, 8, 256) == (7, 0, 1, 8, 1, 28_672, 4, 0, 0, 0, 700, 84)
    # ... and one per lane group at the least
    assert lp.ddc_plan(WR_NCO_ROTATE, False, 0, 7, 1, 8, 256) == (7, 0, 1, 8, 1, 28_672, 4, 0, 0, 0, 7, 7)
    # the cap first: 256 CUs * 4 = 1 024 -> 1 022
    assert lp.ddc_plan(WR_NCO_ROTATE, False, 0, 7, 10_000, 8, 256).wgs == 1_022


def test_ddc_plan_exact_and_split():
    # EXACT: 16 waves, two workgroups per CU, windows only: 16 * 2 * 512 = 16 384; no roles: 40 000 units -> 2 500 -> 512
    assert lp.ddc_plan(WR_NCO_EXACT, False, 0, 4, 10_000, 400, 256) == (4, 0, 1, 16, 1, 16_384, 2, 0, 0, 0, 40_000, 512)
    # SPLIT: the replicated tables: 2 * 256 * 32 * 8 = 131 072, + 16 384; one workgroup per CU
    assert lp.ddc_plan(WR_NCO_SPLIT, True, 0, 4, 10_000, 400, 256) == (4, 0, 1, 16, 1, 147_456, 1, 0, 0, 0, 40_000, 256)


def test_ddc_plan_beyond_sixteen_groups():
    # 18 lane groups: 16 in this launch (never NG = 2: the rest goes out in a launch of its own), two left
    p = lp.ddc_plan(WR_NCO_ROTATE, True, 0, 18, 10_000, 400, 256)
    assert (p.ngroups, p.rest, p.ng) == (16, 0b11 << 16, 1)
    p = lp.ddc_plan(WR_NCO_ROTATE, True, 0, 18, 10_000, 400, 256, gsel=p.rest)
    assert (p.ngroups, p.rest, p.ng) == (2, 0, 1)           # 10 000 * 1 < 4 * 6 144
    assert lp.ddc_plan(WR_NCO_ROTATE, True, 0, 18, 10_000, 400, 256, gsel=1 << 20).ngroups == 0


def test_long_filter_plan():
    # ROTATE, one filter, 4 groups, 128 taps, the post stage riding: two lane groups per wave: 20 000 units -> 2 500 -> 256 * 3
    # roll: 127 * 256 = 32 512 entries / 512 -> 64; LDS: (512 + 8 * 128) * 8 + 8 * 64 * 4 = 14 336 against the post stage's 40 000
    assert lp.long_plan(True, True, 10_000, 4, 128, 256, 256, 5, 63, 4) == (True, True, 768, 256, 64, 40_000, 0, 0)
    # ... nothing riding, an odd group count: 30 000 units -> 3 750 -> 256 * 4
    assert lp.long_plan(True, True, 10_000, 3, 128, 192, 256) == (True, False, 1024, 0, 48, 14_336, 0, 0)
    assert lp.long_plan(True, False, 10, 4, 256, 2048, 256) == (True, False, 5, 0, 256, 14_336, 0, 0)    # 255 * 2 048 / 512 = 1 020
    # the reference's arithmetic: 300 units in fours; the roll: 255 * 192 = 48 960 / 256 -> 192
    assert lp.long_plan(False, False, 100, 3, 256, 192, 256) == (False, False, 0, 0, 0, 0, 75, 192)
    assert lp.long_plan(False, False, 100_000, 16, 256, 1024, 256) == (False, False, 0, 0, 0, 0, 2048, 1020)
    # a block without an output frame: the roll is all there is, in either mode
    assert lp.long_plan(True, True, 0, 4, 128, 256, 256) == (False, False, 0, 0, 0, 0, 0, 127)


def test_audio_filter_plan():
    # D2 = 5, 64 taps: (352 - 64) / 5 + 1 = 58 frames would fit: 16; 15 * 5 + 64 = 139 rows; (139 + 64) * 64 + 16 * 65 floats
    assert lp.audio_plan(2000, 5, 64) == (16, 139, 56_128, 159_808, 125)
    # D2 = 10, 256 taps: (352 - 256) / 10 + 1 = 10 frames; 9 * 10 + 256 = 346 rows; (346 + 256) * 64 + 1 040 floats
    assert lp.audio_plan(95, 10, 256) == (10, 346, 158_272, 159_808, 10)
    assert lp.audio_plan(17, 1, 64) == (16, 79, 40_768, 159_808, 2)
    assert lp.lib().wr_plan_grid_for(0, 256, 2048) == 1 and lp.lib().wr_plan_grid_for(257, 256, 2048) == 2
    assert lp.lib().wr_plan_grid_for(1 << 40, 256, 2048) == 2048


# ---- what holds whatever the shape ---------------------------------------------------------------------------------------
KERNELS = [(WR_NCO_ROTATE, True), (WR_NCO_ROTATE, False), (WR_NCO_SPLIT, True), (WR_NCO_EXACT, False)]


@pytest.mark.parametrize("num_cus", [8, 32, 256])
def test_ddc_plan_invariants(num_cus):
    for nco, utaps in KERNELS:
        for pd2 in ([0] + D2S if nco == WR_NCO_ROTATE else [0]):
            for groups in range(1, 17):
                for k1 in (0, 1, 63, 64, 65, 1000, 10_000):
                    for d1, one_filter in ((1, True), (8, False), (400, True)):
                        p = lp.ddc_plan(nco, utaps, pd2, groups, k1, d1, num_cus, one_filter=one_filter, post_ntiles=7,
                                        post_groups=groups)
                        at = (nco, utaps, pd2, groups, k1, d1, one_filter, p)
                        w = p.waves
                        assert p.ngroups == groups and p.ng in (1, 2), at
                        lowest = groups if (nco == WR_NCO_ROTATE and not utaps) else -(-(groups // p.ng) // w)
                        assert p.wgs >= -(-(groups // p.ng) // w), at
                        assert p.wgs <= max(num_cus * p.wgs_per_cu, lowest), at
                        assert p.wgs_per_cu >= 1, at
                        if p.ng == 2:
                            assert groups % 2 == 0 and one_filter and nco == WR_NCO_ROTATE and utaps, at
                        assert p.kslow <= k1 and p.n_bnd * w >= p.kslow * groups, at
                        assert p.units == (k1 - p.kslow) * (groups // p.ng), at
                        assert p.lds <= CU_LDS and p.lds * p.wgs_per_cu <= CU_LDS, at
                        assert p.post_wgs == (8 * groups if pd2 else 0), at


def test_tilings_cover_every_tile_once():
    """ntiles x run >= tiles > (ntiles - 1) x run, for the three rules"""
    def covers(tiles, run, ntiles):
        return run >= 1 and ntiles * run >= tiles > (ntiles - 1) * run

    for tiles in list(range(1, 70)) + [125, 255, 256, 257, 500, 1023, 4096, 5000]:
        for groups in range(1, 17):
            assert covers(tiles, *lp.post_tiling_riding(tiles, groups)), (tiles, groups)
            for nseg in (1, 2, 4):
                assert covers(tiles, *lp.post_tiling_alone(tiles, groups, nseg)), (tiles, groups, nseg)
            for n_post in (1, 4, 7, 8, 28, 252):
                t = lp.stream_tiling(16 * tiles, groups, n_post)
                at = (tiles, groups, n_post, t)
                assert t.tiles == tiles and covers(tiles, t.run, t.ntiles) and covers(tiles, t.drain_run, t.drain_ntiles), at
                assert t.drain_run == t.min_run <= t.run <= tiles, at
                # every task of the short runs has a post workgroup of its own, unless a lane group's tiles are one task already
                assert t.drain_ntiles * groups <= n_post or t.min_run == tiles, at


# ---- the spectrum launches ------------------------------------------------------------------------------------------------
# A transform of `points` complex points (the frame's n; a real frame's n / 2 packed ones) is a single pass up to 8192 points --
# two LDS buffers of 64 KiB -- and n1 x n2 above, n1 = 2^ceil(bits / 2); sub = max(n1, n2).  65536 IQ points: the register path.
SINGLE, FOUR, REG = lp.FFT_SINGLE, lp.FFT_FOUR_STEP, lp.FFT_REG64K
KIB = 1024


def test_fft_constants():
    assert lp.fft_constants() == dict(threads=256, lds_points=8192, p1_long_min=96, db_grid_cap=1024, waterfall_grid_cap=4096)
    # k_bins_to_db strides from 1024 * 256 bins on; k_waterfall_row never does: 2^20 / 256 = 4096 is the widest row there is
    g = lp.lib().wr_plan_grid_for
    assert [g(n, 256, 1024) for n in (8, 256, 257, 262144, 524288, 1 << 20)] == [1, 1, 2, 1024, 1024, 1024]
    assert [g(w, 256, 4096) for w in (1, 512, 65536, 1 << 20)] == [1, 2, 256, 4096]


@pytest.mark.parametrize("n,real,n1,n2,path", [
    (8, False, 8, 1, SINGLE), (8192, False, 8192, 1, SINGLE),
    (16384, False, 128, 128, FOUR),         # 14 bits: 2^7
    (32768, False, 256, 128, FOUR),         # 15 bits: 2^8
    (65536, False, 256, 256, REG),
    (131072, False, 512, 256, FOUR),        # 17 bits: 2^9
    (262144, False, 512, 512, FOUR),
    (524288, False, 1024, 512, FOUR),       # 19 bits: 2^10
    (1048576, False, 1024, 1024, FOUR),
    # real: the shape of n / 2 points
    (8, True, 4, 1, SINGLE), (16384, True, 8192, 1, SINGLE),
    (32768, True, 128, 128, FOUR), (65536, True, 256, 128, FOUR),
    (131072, True, 256, 256, FOUR),         # 65536 packed points: the register path is for IQ frames only
    (1048576, True, 1024, 512, FOUR),
])
def test_fft_shape(n, real, n1, n2, path):
    s = lp.fft_shape(n, real)
    assert s == (n // 2 if real else n, n1, n2, 0 if n2 == 1 else max(n1, n2), path, 128 * KIB, real)


def test_fft_single_pass_launch():
    # both buffers: 2 * points * 8 bytes; a workgroup per frame
    assert lp.fft_launch(8192, 5) == (0, 0, 0, 128 * KIB, 0, (5, 1), (0, 0), (0, 0))
    assert lp.fft_launch(8, 300) == (0, 0, 0, 128, 0, (300, 1), (0, 0), (0, 0))
    assert lp.fft_launch(16384, 7, real=True) == (0, 0, 0, 128 * KIB, 0, (7, 1), (0, 0), (0, 0))
    assert lp.fft_launch(16, 1, real=True) == (0, 0, 0, 128, 0, (1, 1), (0, 0), (0, 0))


@pytest.mark.parametrize("n,real,want", [
    # ct = min(16, 8192 / n1), rt = min(16, 8192 / n2); lds = 2 * n1 * ct * 8, 2 * n2 * rt * 8; grids (n2 / ct, 5), (n1 / rt, 5)
    (16384, False, (16, 16, 0, 32 * KIB, 32 * KIB, (8, 5), (8, 5), (0, 0))),                # 128 x 128
    (32768, False, (16, 16, 0, 64 * KIB, 32 * KIB, (8, 5), (16, 5), (0, 0))),               # 256 x 128
    (131072, False, (16, 16, 0, 128 * KIB, 64 * KIB, (16, 5), (32, 5), (0, 0))),            # 512 x 256
    (262144, False, (16, 16, 0, 128 * KIB, 128 * KIB, (32, 5), (32, 5), (0, 0))),           # 512 x 512
    (524288, False, (8, 16, 0, 128 * KIB, 128 * KIB, (64, 5), (64, 5), (0, 0))),            # 1024 x 512: 8192 / 1024 = 8 columns
    (1048576, False, (8, 8, 0, 128 * KIB, 128 * KIB, (128, 5), (128, 5), (0, 0))),          # 1024 x 1024
    # real: the untangle step's grid (m / 256, 5) behind them
    (32768, True, (16, 16, 0, 32 * KIB, 32 * KIB, (8, 5), (8, 5), (64, 5))),                # m = 16384: 128 x 128
    (131072, True, (16, 16, 0, 64 * KIB, 64 * KIB, (16, 5), (16, 5), (256, 5))),            # m = 65536: 256 x 256, generic
    (1048576, True, (8, 16, 0, 128 * KIB, 128 * KIB, (64, 5), (64, 5), (2048, 5))),         # m = 524288: 1024 x 512
])
def test_fft_four_step_launch(n, real, want):
    assert lp.fft_launch(n, 5, real) == want


@pytest.mark.parametrize("batch,fpw,rows", [(1, 1, 1), (95, 1, 95), (96, 4, 24), (97, 4, 25), (256, 4, 64), (259, 4, 65)])
def test_fft_register_path_launch(batch, fpw, rows):
    """four frames per pass-1 workgroup from 96 frames on (ceil(batch / 4) rows of 16 workgroups), else one; static LDS"""
    assert lp.fft_launch(65536, batch) == (0, 0, fpw, 0, 0, (16, rows), (16, batch), (0, 0))


def test_fft_lds_and_tiles_at_every_size():
    for real in (False, True):
        for bits in range(3, 21):
            n = 1 << bits
            s = lp.fft_shape(n, real)
            assert s.n1 * s.n2 == s.points and s.n1 >= s.n2 and s.lds_max == 128 * KIB, (n, real, s)
            l = lp.fft_launch(n, 3, real)
            assert l.lds1 <= s.lds_max and l.lds2 <= s.lds_max, (n, real, l)
            if s.path == SINGLE:
                assert s.points <= 8192 and l.lds1 == 16 * s.points, (n, real, l)
            elif s.path == FOUR:
                assert s.points > 8192 and 1 <= l.ct <= 16 and 1 <= l.rt <= 16, (n, real, l)
                assert l.grid1 == (s.n2 // l.ct, 3) and l.grid1[0] * l.ct == s.n2, (n, real, l)
                assert l.grid2 == (s.n1 // l.rt, 3) and l.grid2[0] * l.rt == s.n1, (n, real, l)
                assert l.grid3 == ((s.points // 256, 3) if real else (0, 0)), (n, real, l)
            else:
                assert (n, real) == (65536, False)


def test_fft_work_area():
    # 128 MB of frames of 8 n bytes (IQ and real alike), the batch at most, one frame at least; it only ever grows
    assert lp.fft_work_frames(65536, 1, 1000) == 256 and lp.fft_work_frames(1 << 20, 1, 1000) == 16
    assert lp.fft_work_frames(16384, 1, 7) == 7 and lp.fft_work_frames(16384, 1, 5000) == 1024
    assert lp.fft_work_frames(65536, 100, 5) == 100 and lp.fft_work_frames(65536, 256, 1000) == 256
    assert lp.fft_work_frames(65536, 1, 0) == 1 and lp.fft_work_frames(65536, 0, 0) == 0        # nothing asked for: as it was
    assert lp.fft_work_frames(1 << 25, 0, 5) == 1           # (a frame larger than the cap: one frame)
    assert lp.fft_chunks(65536, 259) == [256, 3] and lp.fft_chunks(65536, 256) == [256] and lp.fft_chunks(65536, 5) == [5]
    assert lp.fft_chunks(1 << 20, 17) == [16, 1] and lp.fft_chunks(1 << 20, 33) == [16, 16, 1]
    assert lp.fft_chunks(32768, 5, have=100) == [5]
    assert lp.fft_chunks(1 << 20, 3, have=1) == [3] and lp.fft_chunks(1 << 20, 0) == []
    # a push (one frame) after a batch of 100 still runs as one batch of one
    assert lp.lib().wr_plan_fft_chunk(1, 100) == 1
    # real: the packed transform lies behind the intermediates of all the frames in flight: work_frames * m points in
    assert lp.lib().wr_plan_fft_untangle_offset(16, 524288) == 8_388_608 and lp.lib().wr_plan_fft_untangle_offset(1, 16384) == 16384


@pytest.mark.parametrize("n,cols,num_cus,ct", [
    # min(8192 / n, 8, cols / CUs) rounded down to a power of two, one at least
    (512, 256, 256, 1),                     # no more columns than compute units
    (512, 4096, 256, 8),
    (8192, 64, 256, 1), (8192, 4096, 8, 1), (8192, 4096, 0, 1),     # the LDS holds one
    (2048, 1024, 256, 4),                   # the LDS holds four
    (64, 768, 256, 2),                      # three per compute unit: two
    (64, 64, 256, 1),
    # num_cus = 0: the rule without the compute units
    (64, 64, 0, 8), (512, 256, 0, 8), (2048, 64, 0, 4), (4096, 64, 0, 2),
])
def test_fft_columns_per_workgroup(n, cols, num_cus, ct):
    assert lp.fft_cols_ct(n, cols, num_cus) == ct
    assert 64 % ct == 0 and 2 * n * ct * 8 <= 128 * KIB


# ==== the voice bank and the row kernels =====================================================================================

def test_voice_plan():
    # a workgroup is one wave of 64 threads, four outputs each: 256 outputs; one workgroup more per row for its history
    assert lp.voice_plan(1) == (64, 4, 256, 8, 2048, 16, 4 + 256 + 2048, 1, 2)
    assert lp.voice_plan(256)[-2:] == (1, 2)
    assert lp.voice_plan(257)[-2:] == (2, 3)
    assert [T for T in (4, 6, 8, 10, 12, 2044, 2046, 2048, 2052) if lp.lib().wr_plan_voice_len_ok(T)] == [8, 12, 2044, 2048]


def test_agc_plan():
    # 256 threads of 4 frames: tiles of 1024, four waves (the grid is a workgroup per row: no arithmetic)
    assert lp.agc_plan() == (256, 4, 1024, 4)


# ---- levels: groups of 256 rows; the work area is sums, peaks and muted counts [groups][cols] each, then the result [3][cols]
@pytest.mark.parametrize("cols,k1,want", [
    # one row: one group; 5 columns are one lane group, one workgroup of k_levels_sum; 3 * 5 + 3 * 5 floats
    (5, 1, dict(groups=1, grid_y=1, sum_grid=1, psum=0, ppeak=5, pmuted=10, res=15, work_floats=30)),
    # 256 rows are still one group; 64 columns still one lane group
    (64, 256, dict(groups=1, grid_y=1, sum_grid=1, psum=0, ppeak=64, pmuted=128, res=192, work_floats=384)),
    # 257 rows: a second group of one row; 300 columns: 5 lane groups, 2 workgroups of 256 for the sum; 3 * 600 + 900
    (300, 257, dict(groups=2, grid_y=5, sum_grid=2, psum=0, ppeak=600, pmuted=1200, res=1800, work_floats=2700)),
])
def test_levels_plan(cols, k1, want):
    p = lp.levels_plan(cols, k1)
    assert (p.rows, p.threads, p.lds_squelch) == (256, 1024, 256 * 64 * 4)
    assert {k: getattr(p, k) for k in want} == want


# ---- the tone bank ----
def test_tones_plan():
    # a workgroup is 4 waves of 128 frames; the push is nq windows and nr frames
    assert lp.tones_plan(1, 16) == (256, 512, 4096, 1, 0, 1)
    assert lp.tones_plan(512, 16) == (256, 512, 4096, 1, 32, 0)
    assert lp.tones_plan(513, 16) == (256, 512, 4096, 2, 32, 1)
    assert lp.tones_plan(1 << 28, 65536) == (256, 512, 4096, 1 << 19, 4096, 0)


# a row with `fill` frames in its open window takes n frames: ends = (fill + n) / W windows end, the last of them at frame
# e = ends * W - fill of the push; A = [max(e - W, 0), e) counted from oa = e - W, B = [e, n) counted from e; no end: B is
# the push, counted from -fill
@pytest.mark.parametrize("fill,n,W,want", [
    # fill + n < W: no end
    (5, 10, 16, dict(a_lo=0, b_lo=0, oa=0, ob=-5, ends=0, fill_after=15)),
    (65000, 500, 65536, dict(a_lo=0, b_lo=0, oa=0, ob=-65000, ends=0, fill_after=65500)),
    # fill + n == W: e = 16 - 5 = 11 = n, the window began 5 frames before the push
    (5, 11, 16, dict(a_lo=0, b_lo=11, oa=-5, ob=11, ends=1, fill_after=0)),
    (0, 16, 16, dict(a_lo=0, b_lo=16, oa=0, ob=16, ends=1, fill_after=0)),
    (65000, 536, 65536, dict(a_lo=0, b_lo=536, oa=-65000, ob=536, ends=1, fill_after=0)),
    # one end, fill > 0: oa negative, a_lo = 0; 5 + 20 = 16 + 9
    (5, 20, 16, dict(a_lo=0, b_lo=11, oa=-5, ob=11, ends=1, fill_after=9)),
    (1, 65536, 65536, dict(a_lo=0, b_lo=65535, oa=-1, ob=65535, ends=1, fill_after=1)),
    # several ends: 5 + 45 = 3 * 16 + 2, e = 48 - 5 = 43, the last whole window is [27, 43); the two before it only count
    (5, 45, 16, dict(a_lo=27, b_lo=43, oa=27, ob=43, ends=3, fill_after=2)),
    # 65535 + 131073 = 3 * 65536, e = 196608 - 65535 = 131073
    (65535, 131073, 65536, dict(a_lo=65537, b_lo=131073, oa=65537, ob=131073, ends=3, fill_after=0)),
    # the longest push: 100 + 2^28 = 4096 * 65536 + 100, e = 2^28 - 100
    (100, 1 << 28, 65536, dict(a_lo=(1 << 28) - 100 - 65536, b_lo=(1 << 28) - 100, oa=(1 << 28) - 100 - 65536,
                                ob=(1 << 28) - 100, ends=4096, fill_after=100)),
])
def test_tones_cut(fill, n, W, want):
    assert lp.tones_cut(fill, n, W)._asdict() == want


def test_tones_cut_counts_as_the_restatement_does():
    """every fill < W and n < 3 W at W = 16: windows ended and the fill left are tests/tones_np.py's, and the stretches
    lie inside the push in order"""
    import numpy as np
    import tones_np
    W = 16
    for fill in range(W):
        for n in range(1, 3 * W):
            bank = tones_np.Bank(1, [1 << 20], W)
            bank.fill[0] = fill
            bank.push(np.zeros((1, n), np.float32))
            c = lp.tones_cut(fill, n, W)
            assert (c.ends, c.fill_after) == (int(bank.windows[0]), int(bank.fill[0])), (fill, n)
            assert 0 <= c.a_lo <= c.b_lo <= n and c.oa <= c.a_lo and c.ob <= c.b_lo, (fill, n)
            assert c.a_lo - c.oa < W and n - c.ob <= W and (c.b_lo - c.oa == W if c.ends else c.b_lo == 0), (fill, n)


# ---- the DCS bank: the clock is frames * step in units of 2^-29 chip; a launch may touch DC_SPAN = 256 chips ----
@pytest.mark.parametrize("first_frame,step,nframes", [
    (0, 1 << 19, 1 << 28),                  # 1024 frames a chip: 2^18 frames a launch, 1024 launches
    (12345, 1 << 19, 300_000),
    (0, 1 << 28, 100_000),                  # 2 frames a chip: 511 frames a launch from a chip's start
    (7, 1 << 28, 100_000),                  # ... and 510 from its middle
    ((1 << 46) + 3, 1 << 19, 1 << 20),      # first_frame * step = 2^65 + ...: beyond 64 bits
    ((1 << 37) + 1, 1 << 28, 5_000),        # 2^65 + 2^28
    ((1 << 40) + 11, (1 << 28) - 1, 50_000),
    (3, 1 << 28, 1), (3, 1 << 19, 510),
])
def test_dcs_launches(first_frame, step, nframes):
    span = lp.dcs_constants()["span"]
    assert span == 256
    runs = lp.dcs_launches(first_frame, step, nframes)
    at = first_frame * step                                     # Python's integers do not wrap
    for g0, ph0, n, room in runs:
        assert (g0, ph0) == (at >> 29, at & ((1 << 29) - 1))
        assert 1 <= n <= room and room >= 510
        assert (ph0 + n * step) >> 29 < span                    # the chip of the frame behind the launch included
        assert (ph0 + (room + 1) * step) >> 29 >= span          # ... and room is the most that keeps it so
        at += n * step
    assert sum(r.frames for r in runs) == nframes
    assert all(r.frames == r.room for r in runs[:-1])           # only the last launch is short


def test_dcs_least_room_is_510():
    # step 2^28 and a launch that begins half a chip in: (256 * 2^29 - 1 - 2^28) / 2^28 = 511 - 1 / 2^28 -> 510
    assert [r.room for r in lp.dcs_launches(1, 1 << 28, 2)] == [510]
    assert [r.room for r in lp.dcs_launches(0, 1 << 28, 2)] == [511]
    assert [r.room for r in lp.dcs_launches(0, 1 << 19, 2)] == [(1 << 18) - 1]
    L = lp.lib()
    assert [s for s in ((1 << 19) - 1, 1 << 19, 1 << 28, (1 << 28) + 1) if L.wr_plan_dcs_step_ok(s)] == [1 << 19, 1 << 28]


# ---- the resampler ----
RESAMP_SHAPES = [(1, 8, 64), (1024, 8192, 4), (1024, 128, 16), (3, 2, 4), (441, 500, 32)]


def test_resamp_limits():
    assert lp.resamp_constants() == dict(threads=256, span=2112, l_max=1024, ratio_max=8, p_min=4, p_max=64, taps_max=16384)
    bad = lp.lib().wr_plan_resamp_limits_bad
    assert not any(bad(*s) for s in RESAMP_SHAPES)
    # L of 0 and above 1024, M above 8 L, L above 8 M, P of 0, above 64, no multiple of 4, L * P above 16384
    assert all(bad(*s) for s in [(0, 1, 4), (1025, 1025, 4), (1, 9, 4), (9, 1, 4), (1, 1, 0), (1, 1, 68), (1, 1, 6),
                                 (1024, 1024, 20), (1, 0, 4)])


@pytest.mark.parametrize("L,M,P", RESAMP_SHAPES)
def test_resamp_out_frames_over_cuts_of_a_stream(L, M, P):
    """however a stream of N frames is cut into pushes, the pushes' output frames sum to ceil(N L / M), each as
    tests/resamp_np.py has it"""
    import numpy as np
    import resamp_np
    for cuts in ([1] * 40, [M - 1, 1, M, M + 1, 1], [7, 300, 1, 1, 5000, 13], [1 << 28, 1, (1 << 28) - 1]):
        ref = resamp_np.Bank(1, L, M, np.zeros((L, P), np.float32))
        nmod = total = 0
        for n in cuts:
            got = lp.resamp_out_frames(L, M, nmod, n)
            assert got == ref.out_frames(n) == lp.resamp_plan(L, M, nmod, n).n_out
            total += got
            nmod = ref.nmod = (nmod + n) % M
        N = sum(cuts)
        assert total == -(-N * L // M)


def _resamp_chunks_hold(L, M, P, nmod, n):
    """the plan of a push against the closed form: output 256 i of the push is output j0 + 256 i since the clock was last
    a multiple of M, at t = (j0 + 256 i) M: input frame t / L - nmod of the push, phase t mod L"""
    p = lp.resamp_plan(L, M, nmod, n)
    j0 = -(-nmod * L // M)
    assert p.j0 == j0 and p.chunks == -(-p.n_out // 256) and p.grid_x == p.chunks + 1
    worst = 0
    for i in sorted({0, 1, p.chunks // 2, p.chunks - 1} & set(range(p.chunks))):
        c = lp.resamp_chunk(L, M, P, nmod, n, i)
        t = (j0 + 256 * i) * M
        assert (c.i0, c.base, c.rem0, c.lo) == (256 * i, t // L - nmod, t % L, t // L - nmod - (P - 1)), (nmod, n, i)
        assert c.cnt == min(256, p.n_out - 256 * i) >= 1
        # the last output of the chunk reads up to frame (t + (cnt - 1) M) / L of the push, the first from P - 1 before base
        assert c.span == (t + (c.cnt - 1) * M) // L - t // L + P
        assert 0 <= c.base and c.lo + c.span <= n and c.span <= lp.resamp_constants()["span"]
        worst = max(worst, c.span)
    return worst


@pytest.mark.parametrize("L,M,P", RESAMP_SHAPES[:4])
def test_resamp_chunks(L, M, P):
    worst = max(_resamp_chunks_hold(L, M, P, nmod, n) for nmod in sorted({0, 1, M // 2, M - 1} & set(range(M)))
                for n in (1, M, 8 * 256 + 1, 100_000))
    if (L, M, P) == (1, 8, 64):
        assert worst == 2104                                    # (0 + 255 * 8) / 1 + 64: the longest span there is


def test_resamp_chunks_at_every_clock():
    for nmod in range(500):
        _resamp_chunks_hold(441, 500, 32, nmod, 3000)


def test_resamp_chunk_by_hand():
    # 3 / 2, P = 4, the clock at 1, 1000 frames: j0 = ceil(3 / 2) = 2, ceil(1001 * 3 / 2) - 2 = 1500 outputs, 6 chunks;
    # chunk 5: t = (2 + 1280) * 2 = 2564 = 3 * 854 + 2: frame 854 - 1 of the push, phase 2; 220 outputs; (2 + 219 * 2) / 3 + 4
    assert lp.resamp_plan(3, 2, 1, 1000) == (1500, 2, 6, 7)
    assert lp.resamp_chunk(3, 2, 4, 1, 1000, 5) == (1280, 853, 850, 2, 220, 150)
