"""The frame driver's decisions, one rule per test, on the CPU (csrc/gsr_frame_plan.h through gsr_debug_frame_plan).  Which regime a
frame takes -- culled, front slab, cached order, small-frame sort -- and how frame_finish ends an attempt from what its mailbox said
(csrc/gsr_mailbox.h).  No regime can change a pixel (the GPU exactness tests and the soak prove that); what is pinned here is WHEN the
library takes which path.  Flat int32 layouts, field for field the X-lists of the header: no context, no GPU."""
import numpy as np
import pytest

PLAN_IN = ("phase_in", "allow_cull", "out_is_device", "has_depth", "n", "nclus", "sh_order", "key_min", "key_max",
           "opt_deferred", "opt_lazy", "opt_cull", "opt_slab", "opt_cluster", "opt_sort_cache", "opt_local_sort", "opt_k1_scatter",
           "opt_scatter_direct", "opt_mid_sort", "opt_bn_items", "full_keys", "shard_count", "timing", "timing_all", "opt_timing",
           "lazy_pays", "prefix_cheaper", "prefix_valid", "bbox_ok", "horizon_match", "hpyr_re", "sort_match", "sorted_culled",
           "sorted_dculled", "pos_match", "same_pos", "jumped")
HINTS = ("surv_hint", "kept_hint", "kept_lo", "kept_hi", "kept_culled", "slab_kept", "slab_kept1", "slab_kept2")
PLAN_OUT = ("deferred", "lazy", "cull", "jumped", "cull_dilate", "phase", "timing", "timing_all", "dcull", "cache_hit", "want_pos",
            "ordered", "key_bits", "n_slots", "held", "local", "local_phase", "k1_scatters", "bk_lo", "bk_shift", "scatter_direct",
            "mid_sort", "k1_grid", "bn_items", "bn_blocks", "bn_grid", "classic_once")
OUT_IN = ("has_splats", "phase", "cull", "local_sort", "dcull", "dblind", "speculative", "deferred", "blend_guess_plain", "key_min",
          "pair_cap", "has_list_buffer", "max_pairs", "mb_pairs", "mb_hints", "mb_kept", "mb_clusters", "mb_key_lo", "mb_key_hi")
OUT_OUT = ("end", "back_end", "grow", "guard_miss", "local_result", "depth_active", "verdicts", "kept_counts", "slab_done") + HINTS
DONE, PHASE_2, SORT_GAVE_UP, DEPTH_APPEARED, SLAB_OVERRUN, TOO_MANY_PAIRS = range(6)
BE_KEPT, BE_QUEUED, BE_REQUEUED, BE_TRUNCATED = range(4)
SORT_GAVE_UP_BIT, DEPTH_COVERED_BIT = 32, 64
KEY_MIN = 0x3e000000

# a 6 M-splat cloud at 1080p under the library's default options, its slot's previous frame unculled and known
FRAME = dict(phase_in=0, allow_cull=1, out_is_device=1, has_depth=0, n=6_000_000, nclus=93_750, sh_order=3, key_min=KEY_MIN,
             key_max=KEY_MIN + (1 << 22), opt_deferred=0, opt_lazy=1, opt_cull=1, opt_slab=1, opt_cluster=1, opt_sort_cache=1,
             opt_local_sort=1, opt_k1_scatter=1, opt_scatter_direct=1, opt_mid_sort=1, opt_bn_items=0, full_keys=0, shard_count=1,
             timing=1, timing_all=0, opt_timing=1, lazy_pays=0, prefix_cheaper=0, prefix_valid=1, bbox_ok=1, horizon_match=1, hpyr_re=2,
             sort_match=0, sorted_culled=0, sorted_dculled=0, pos_match=0, same_pos=0, jumped=0,
             surv_hint=40_000, kept_hint=2_000_000, kept_lo=KEY_MIN + 1000, kept_hi=KEY_MIN + 900_000, kept_culled=0, slab_kept=0,
             slab_kept1=0, slab_kept2=0, classic_once=0)
# an attempt of an ordinary speculative frame whose mailbox came back with nothing unusual in it
ATTEMPT = dict(has_splats=1, phase=0, cull=0, local_sort=0, dcull=0, dblind=0, speculative=1, deferred=0, blend_guess_plain=0,
               key_min=KEY_MIN, pair_cap=10_000_000, has_list_buffer=1, max_pairs=0x7fffff00, mb_pairs=8_000_000, mb_hints=0,
               mb_kept=1_500_000, mb_clusters=30_000, mb_key_lo=500, mb_key_hi=700_000,
               surv_hint=1, kept_hint=1, kept_lo=1, kept_hi=2, kept_culled=0, slab_kept=0, slab_kept1=0, slab_kept2=0)


def policy_state(pays=1, vis_unculled=2_000_000, cull_holdoff=0, slab_holdoff=0, local_fails=0, local_holdoff=0, dilate=2):
    return np.array([pays, 0, vis_unculled, cull_holdoff, 8, 0, dilate, 2, slab_holdoff, local_fails, local_holdoff, 0, 0, 0, 0, 0], np.int32)


@pytest.fixture
def L(pkg):
    return pkg.load_library()


def plan(L, policy=None, **kw):
    v = dict(FRAME, **kw)
    pol = policy_state() if policy is None else policy
    inp = np.array([v[k] & 0xffffffff for k in PLAN_IN + HINTS + ("classic_once",)], np.uint32).view(np.int32)
    out = np.zeros(len(PLAN_OUT), np.int32)
    assert L.gsr_debug_frame_plan(0, inp.ctypes.data, pol.ctypes.data, out.ctypes.data) == 0
    return {k: int(x) for k, x in zip(PLAN_OUT, out)}


def outcome(L, **kw):
    v = dict(ATTEMPT, **kw)
    inp = np.array([v[k] & 0xffffffff for k in OUT_IN + HINTS], np.uint32).view(np.int32)
    out = np.zeros(len(OUT_OUT), np.int32)
    assert L.gsr_debug_frame_plan(1, inp.ctypes.data, None, out.ctypes.data) == 0
    return {k: int(np.uint32(x)) if k in HINTS else int(x) for k, x in zip(OUT_OUT, out)}


def test_the_door_refuses_an_unknown_selector(L):
    z = np.zeros(64, np.int32)
    assert L.gsr_debug_frame_plan(2, z.ctypes.data, z.ctypes.data, z.ctypes.data) != 0


def test_an_ordinary_frame_culls_against_the_slot_horizons_and_sorts_with_the_global_passes(L):
    p = plan(L)
    assert p["cull"] == 1 and p["phase"] == 0 and p["cache_hit"] == 0 and p["local"] == 0 and p["ordered"] == 0
    assert p["cull_dilate"] == 0                      # (dilate 2, both built into the slot's pyramid)
    assert p["key_bits"] == 23 and p["n_slots"] == 23_438 * 256
    assert p["bn_items"] == 4 and p["k1_grid"] == (10_000 * 5 // 4 + 64)


def test_a_static_redraw_hits_the_cache_and_then_takes_neither_slab_nor_local_sort(L):
    kw = dict(horizon_match=0, sort_match=1, kept_hint=100_000)    # (a small kept set: the small-frame sort would be predicted)
    p = plan(L, **kw)
    assert p["cache_hit"] == 1 and p["phase"] == 0 and p["local"] == 0 and p["local_phase"] == 0
    assert plan(L, **dict(kw, sort_match=0))["phase"] == 1       # the same frame without a cached order takes a front slab
    pol = policy_state(local_holdoff=5)
    plan(L, pol, **kw)
    assert pol[10] == 5                                          # (a static redraw does not wear the small-frame sort's back-off down)


def test_a_culled_frame_never_reuses_a_cached_order(L):
    assert plan(L, sort_match=1)["cull"] == 1 and plan(L, sort_match=1)["cache_hit"] == 0
    assert plan(L, sort_match=1, horizon_match=0, sorted_culled=1)["cache_hit"] == 0    # nor an unculled one a culled frame's order
    assert plan(L, sort_match=1, horizon_match=0, sorted_dculled=1)["cache_hit"] == 0   # nor one culled against its depth buffer


def test_a_camera_jump_drops_culling_in_policy_mode_only(L):
    p = plan(L, jumped=1)
    assert p["cull"] == 0 and p["jumped"] == 1 and p["phase"] == 1       # (then a front slab where that pays)
    p = plan(L, jumped=1, opt_cull=2)
    assert p["cull"] == 1 and p["jumped"] == 0


def test_culling_waits_for_the_policy_and_a_rerender_never_culls_or_ticks(L):
    assert plan(L, policy_state(pays=0))["cull"] == 0
    pol = policy_state(cull_holdoff=3)
    assert plan(L, pol)["cull"] == 0 and pol[3] == 2                     # held off: this frame counts down
    pol = policy_state(cull_holdoff=3)
    p = plan(L, pol, allow_cull=0)
    assert p["cull"] == 0 and pol[3] == 3                                # (frame_check's re-render: no tick)
    assert plan(L, opt_cull=3)["cull"] == 0 and plan(L, full_keys=1)["cull"] == 0


def test_a_front_slab_frame_is_never_deferred_and_phase_2_uses_dilation_0(L):
    p = plan(L, horizon_match=0, opt_deferred=1)
    assert p["deferred"] == 1 and p["phase"] == 0 and p["cull"] == 0
    p = plan(L, horizon_match=0)
    assert p["phase"] == 1 and p["lazy"] == 0 and p["k1_grid"] == 8192 and p["bn_items"] == 2
    assert plan(L, horizon_match=0, opt_deferred=1, out_is_device=0)["phase"] == 1    # (host targets are never deferred)
    p2 = plan(L, phase_in=2, allow_cull=0, opt_deferred=1, hpyr_re=0, policy=policy_state(dilate=8))
    assert p2["phase"] == 2 and p2["cull_dilate"] == 0 and p2["deferred"] == 0 and p2["cull"] == 0
    pol = policy_state(slab_holdoff=10)
    assert plan(L, pol, horizon_match=0)["phase"] == 0 and pol[8] == 9    # a weak slab holds itself off; phase 0 counts it down


def test_timing_of_a_front_slab_frame_brackets_phase_1_blend_only(L):
    p = plan(L, horizon_match=0, timing=1, timing_all=1, opt_timing=2)
    assert p["phase"] == 1 and p["timing"] == 0 and p["timing_all"] == 0
    p = plan(L, horizon_match=0)
    assert p["timing"] == 1 and p["timing_all"] == 0
    assert plan(L, phase_in=2, allow_cull=0)["timing"] == 0


def test_the_small_frame_sort_is_predicted_from_a_small_kept_set_of_the_same_kind(L):
    p = plan(L, kept_hint=300_000, kept_culled=1)
    assert p["local"] == 1 and p["k1_scatters"] == 1 and p["bn_items"] == 2
    margin = (900_000 - 1000) // 16 + 64                    # the kept range widened by a sixteenth on either side ...
    width = 900_000 + margin + 1                            # ... (its low end clamps at key_min)
    assert p["bk_lo"] == 0 and p["bk_shift"] == 10 and width >> 10 <= 1024 < width >> 9
    assert plan(L, kept_hint=100_000, kept_culled=1)["bn_items"] == 1


def test_the_small_frame_sort_is_refused_after_classic_once_and_consumes_it(L):
    p = plan(L, kept_hint=300_000, kept_culled=1, classic_once=1)
    assert p["local"] == 0 and p["classic_once"] == 0
    p = plan(L, horizon_match=0, kept_hint=300_000, classic_once=1, slab_kept1=100_000)
    assert p["phase"] == 1 and p["local_phase"] == 0 and p["classic_once"] == 1     # phase 1 leaves it for its phase 2 ...
    p = plan(L, phase_in=2, allow_cull=0, classic_once=1, slab_kept2=100_000)
    assert p["local_phase"] == 0 and p["classic_once"] == 0                         # ... which consumes it
    assert plan(L, sort_match=1, horizon_match=0, classic_once=1)["classic_once"] == 1   # (a cache hit sorts nothing: kept)


def test_the_small_frame_sort_is_refused_under_back_off(L):
    pol = policy_state(local_fails=3)
    p = plan(L, pol, kept_hint=300_000, kept_culled=1)
    assert p["held"] == 1 and p["local"] == 0 and pol[9] == 0 and pol[10] == 63
    assert plan(L, policy_state(local_holdoff=5), kept_hint=300_000, kept_culled=1, opt_local_sort=2)["local"] == 1   # (forced)


def test_the_small_frame_sort_is_refused_across_a_culled_unculled_change(L):
    assert plan(L, kept_hint=300_000, kept_culled=0)["local"] == 0       # culled frame, prediction from an unculled one
    assert plan(L, horizon_match=0, opt_slab=0, kept_hint=300_000, kept_culled=1)["local"] == 0
    assert plan(L, horizon_match=0, opt_slab=0, kept_hint=300_000, kept_culled=0)["local"] == 1


def test_the_small_frame_sort_is_refused_below_10_key_bits(L):
    kw = dict(kept_hint=300_000, kept_culled=1, kept_lo=KEY_MIN, kept_hi=KEY_MIN + 500)
    assert plan(L, key_max=KEY_MIN + 511, **kw)["key_bits"] == 9 and plan(L, key_max=KEY_MIN + 511, **kw)["local"] == 0
    assert plan(L, key_max=KEY_MIN + 512, **kw)["key_bits"] == 10 and plan(L, key_max=KEY_MIN + 512, **kw)["local"] == 1
    assert plan(L, phase_in=2, allow_cull=0, key_max=KEY_MIN + 511, slab_kept2=1000)["local_phase"] == 0


def test_deferred_and_full_key_frames_keep_the_global_passes(L):
    assert plan(L, kept_hint=300_000, kept_culled=0, horizon_match=0, opt_deferred=1)["local"] == 0
    assert plan(L, kept_hint=300_000, kept_culled=1, full_keys=1)["local"] == 0


def test_the_position_keyed_order_is_walked_once_the_position_repeats(L):
    kw = dict(opt_sort_cache=2, horizon_match=0)
    assert plan(L, **kw)["want_pos"] == 1 and plan(L, **kw)["ordered"] == 0            # a moving camera never pays for it
    assert plan(L, same_pos=1, **kw)["ordered"] == 1 and plan(L, pos_match=1, **kw)["ordered"] == 1
    assert plan(L, same_pos=1, shard_count=2, **kw)["ordered"] == 0
    p = plan(L, same_pos=1, kept_hint=300_000, **kw)
    assert p["local"] == 0 and p["phase"] == 0 and p["k1_grid"] == 93_750 // 4 + 1     # (K1 walks all slots)


def test_an_empty_cloud_plans_no_grids(L):
    p = plan(L, n=0, nclus=0, horizon_match=0)
    assert p["cull"] == 0 and p["phase"] == 0 and p["n_slots"] == 0 and p["k1_grid"] == 0 and p["bn_items"] == 4 and p["bn_grid"] == 0


def test_lazy_colour_follows_the_kernels_verdict_and_a_culled_frame_the_prefix_verdict(L):
    assert plan(L, horizon_match=0, opt_slab=0, lazy_pays=1)["lazy"] == 1
    assert plan(L, lazy_pays=1)["lazy"] == 0                                   # culled: K1 shades what it keeps ...
    assert plan(L, prefix_cheaper=1)["lazy"] == 1                               # ... unless the list prefixes are cheaper
    assert plan(L, horizon_match=0, opt_slab=0, lazy_pays=1, sh_order=0)["lazy"] == 0


def test_outcome_an_ordinary_frame_keeps_its_back_end_and_leaves_phase_0_hints(L):
    o = outcome(L)
    assert o["end"] == DONE and o["back_end"] == BE_KEPT and o["grow"] == 0 and o["verdicts"] == 1 and o["kept_counts"] == 1
    assert (o["surv_hint"], o["kept_hint"], o["kept_culled"]) == (30_000, 1_500_000, 0)
    assert (o["kept_lo"], o["kept_hi"]) == (KEY_MIN + 500, KEY_MIN + 700_000)
    assert o["local_result"] == -1 and o["depth_active"] == -1
    assert outcome(L, local_sort=1)["local_result"] == 0


def test_outcome_a_phase_1_frame_counts_the_slab_and_continues(L):
    o = outcome(L, phase=1, cull=0, mb_kept=200_000, slab_kept1=7, kept_hint=55)
    assert o["end"] == PHASE_2 and o["verdicts"] == 1 and o["kept_counts"] == 0 and o["slab_done"] == 0
    assert (o["slab_kept"], o["slab_kept1"], o["kept_hint"]) == (200_000, 200_000, 55)
    assert (o["kept_lo"], o["kept_hi"]) == (0, 0)
    assert outcome(L, phase=1, mb_kept=0)["slab_kept1"] == 1                      # (0 = "none yet": an empty slab is 1)


def test_outcome_a_phase_2_frame_predicts_the_next_from_both_phases(L):
    o = outcome(L, phase=2, slab_kept=200_000, mb_kept=300_000, mb_clusters=90_000)
    assert o["end"] == DONE and o["verdicts"] == 0 and o["kept_counts"] == 0 and o["slab_done"] == 1
    assert (o["slab_kept2"], o["kept_hint"], o["kept_culled"]) == (300_000, 500_000, 1)
    assert o["surv_hint"] == max(16384, 2 * (500_000 // 64 + 1))
    assert outcome(L, phase=2, slab_kept=0, mb_kept=1000, mb_clusters=5000)["surv_hint"] == 5000    # (never above what survived)
    assert (o["kept_lo"], o["kept_hi"]) == (0, 0)


def test_outcome_sort_gave_up_keeps_nothing_of_the_attempt(L):
    o = outcome(L, local_sort=1, mb_hints=SORT_GAVE_UP_BIT | 4, kept_hint=9, surv_hint=77)
    assert o["end"] == SORT_GAVE_UP and o["local_result"] == 1 and o["verdicts"] == 0 and o["kept_counts"] == 0
    assert (o["kept_hint"], o["kept_lo"], o["kept_hi"], o["surv_hint"]) == (0, 0, 0, 77)
    assert outcome(L, local_sort=0, mb_hints=SORT_GAVE_UP_BIT)["end"] == DONE     # (the bit means something for that sort only)


def test_outcome_depth_appeared_under_a_blind_culled_frame_renders_it_again(L):
    kw = dict(dcull=1, dblind=1, cull=1, mb_hints=DEPTH_COVERED_BIT)
    o = outcome(L, **kw)
    assert o["end"] == DEPTH_APPEARED and o["depth_active"] == 1 and o["verdicts"] == 0
    o = outcome(L, **dict(kw, cull=0))                                             # unculled: the depth test copes by itself
    assert o["end"] == DONE and o["depth_active"] == 1
    assert outcome(L, dcull=1, dblind=0, cull=1)["depth_active"] == 0


def test_outcome_slab_phase_2_overrunning_its_buffer_renders_the_frame_again(L):
    o = outcome(L, phase=2, mb_pairs=12_000_000)
    assert o["end"] == SLAB_OVERRUN and o["grow"] == 1
    o = outcome(L, phase=2, mb_pairs=12_000_000, speculative=0)                   # (nothing clamped ran: queued once it fits)
    assert o["end"] == DONE and o["back_end"] == BE_QUEUED and o["grow"] == 1


def test_outcome_a_short_buffer_requeues_the_speculative_back_end(L):
    o = outcome(L, mb_pairs=12_000_000)
    assert o["end"] == DONE and o["back_end"] == BE_REQUEUED and o["grow"] == 1
    assert outcome(L, has_list_buffer=0, mb_pairs=0, speculative=0)["grow"] == 1  # (a slot that never met a pair gets a buffer)
    assert outcome(L, speculative=0)["back_end"] == BE_QUEUED


def test_outcome_a_deferred_frame_with_clamped_lists_is_counted_truncated(L):
    assert outcome(L, deferred=1, mb_pairs=12_000_000)["back_end"] == BE_TRUNCATED
    assert outcome(L, deferred=1)["back_end"] == BE_KEPT


def test_outcome_guard_miss_hands_the_frame_to_the_depth_tested_kernel(L):
    kw = dict(dcull=1, blend_guess_plain=1, mb_hints=DEPTH_COVERED_BIT)
    assert outcome(L, **kw)["guard_miss"] == 1
    assert outcome(L, **dict(kw, mb_hints=0))["guard_miss"] == 0
    assert outcome(L, **dict(kw, mb_pairs=12_000_000))["guard_miss"] == 0         # (a requeued back end guesses again, unguarded)


def test_outcome_too_many_pairs_is_an_error_after_the_hints(L):
    o = outcome(L, mb_pairs=0xffffffff)
    assert o["end"] == TOO_MANY_PAIRS and o["kept_hint"] == 1_500_000
    assert outcome(L, mb_pairs=0x7fffff01)["end"] == TOO_MANY_PAIRS


def test_outcome_of_an_empty_frame_reads_no_mailbox(L):
    o = outcome(L, has_splats=0, mb_hints=SORT_GAVE_UP_BIT | DEPTH_COVERED_BIT, local_sort=1, kept_hint=5)
    assert o["end"] == DONE and o["back_end"] == BE_KEPT and o["verdicts"] == 0 and o["local_result"] == -1 and o["kept_hint"] == 5
