"""The environment switches as the sources read them BEFORE rescan_amd/csrc/rs_switches.h existed (commit 3acef66), transcribed by hand
from the ~100 getenv calls of rs_api.hip, rs_icp_estimate.hip and rs_dropin.cpp — not from the new header: tests/test_switches_cpu.py
holds the header to this.

A row: name -> (kind, default, class, setter).
  kind     flag (set at all), int (atoi), i64 (atoll), float ((float)atof), double (atof), word
  class    boot   initialised a file-scope variable when the library was loaded
           first  a function-local `static const`, latched the first time its path ran
           live   read afresh whenever its path ran
  setter   the C entry point that changed the variable afterwards (boot rows), or None

One row differs from the list in the issue that asked for the table: RS_DROPIN_STATS was not read per call but once, by the
initialiser of the shim's file-scope `g_stats` (boot, without a setter)."""

PARENT = {
    # rs_api.hip, file scope
    "RS_HIP_CHAINS_RETRY_AFTER": ("int", 15, "boot", "rs_hip_icp_chains_retry_after"),
    "RS_HIP_REF_ORDER_BELOW": ("int", 16384, "boot", "rs_hip_icp_reference_order_below"),
    "RS_HIP_FAITH_GUESS": ("int", 1000, "boot", "rs_hip_icp_faith_guess"),
    "RS_HIP_EXACT_CENTROIDS": ("int", 1, "boot", "rs_hip_icp_exact_centroids"),
    "RS_HIP_REPLAY_BELOW": ("int", 0, "boot", "rs_hip_icp_replay_below"),
    "RS_HIP_LANE_CHAINS_BELOW": ("int", 65536, "boot", "rs_hip_icp_lane_chains_below"),
    "RS_HIP_STOP_GUARD": ("float", 1.5e-6, "boot", "rs_hip_icp_stop_guard"),
    "RS_HIP_EARLY_PLAIN": ("int", 1, "boot", "rs_hip_icp_early_plain"),
    "RS_HIP_PLAIN_RECORDS": ("int", 0, "boot", "rs_hip_icp_plain_from_records"),
    "RS_HIP_SCORE_SCENE_MIN": ("i64", 65536, "boot", "rs_hip_score_scene_space_from"),
    # rs_icp_estimate.hip, file scope
    "RS_HIP_UPDATE_FENCED": ("int", 0, "boot", "rs_hip_icp_update_fenced"),
    # rs_api.hip, function-local statics
    "RS_HIP_EARLY_TAIL": ("int", 0, "first", None),
    "RS_HIP_PROF_EVERY": ("int", 1, "first", None),
    "RS_HIP_TILE_EXTENT_MAX": ("float", 0.3, "first", None),
    "RS_HIP_AUTO_CELL_SCALE": ("float", 1.0, "first", None),
    "RS_HIP_SOLO_STAGES": ("int", -1, "first", None),
    "RS_HIP_HANDOFF_K": ("int", -1, "first", None),
    "RS_HIP_HEAVY_STREAMED": ("int", 400, "first", None),
    "RS_HIP_HEAVY_HANDOFF": ("int", 600, "first", None),
    "RS_HIP_HEAVY_TOTAL": ("int", 400, "first", None),
    "RS_HIP_CHAIN_REFRESH": ("int", 0, "first", None),
    "RS_HIP_ICP_CHUNK": ("int", 4, "first", None),
    "RS_HIP_COOP_ALL_BELOW": ("i64", 4096, "first", None),
    "RS_HIP_COOP_WAVES": ("int", 0, "first", None),
    "RS_HIP_ICP_BATCH_BYTES": ("double", 4e9, "first", None),
    "RS_HIP_SCORE_SCENE": ("int", 1, "first", None),
    "RS_HIP_SCORE_PARENT": ("float", 1.0, "first", None),
    "RS_HIP_SCORE_NBIN": ("int", 1, "first", None),
    "RS_HIP_SCORE_CULL": ("int", 1, "first", None),
    "RS_HIP_SCORE_SCENE_DENSITY": ("double", 128.0, "first", None),
    "RS_HIP_SCORE_COUNTING": ("int", 22, "first", None),
    "RS_HIP_ROWS_ZERO_COPY_BELOW": ("i64", 256 << 10, "first", None),
    "RS_HIP_ROWS_POLL": ("flag", 0, "first", None),
    # rs_api.hip, read where used
    "RS_HIP_NO_WARM": ("flag", 0, "live", None),
    "RS_HIP_NO_SEED": ("flag", 0, "live", None),
    "RS_HIP_NO_BY_ROWS": ("flag", 0, "live", None),
    "RS_HIP_NO_BOUNDED_ONLY": ("flag", 0, "live", None),
    "RS_HIP_NO_CERT": ("flag", 0, "live", None),
    "RS_HIP_NO_RANK_CERT": ("flag", 0, "live", None),
    "RS_HIP_NO_LPT": ("flag", 0, "live", None),
    "RS_HIP_NO_ROWS_WAVE": ("flag", 0, "live", None),
    "RS_HIP_ROWS_TILED_FROM": ("i64", 4096, "live", None),
    "RS_HIP_DEBUG": ("flag", 0, "live", None),
    "RS_HIP_DEBUG_CYCLES": ("flag", 0, "live", None),
    "RS_HIP_LANE_DEBUG": ("flag", 0, "live", None),
    "RS_HIP_CHAIN_DEBUG": ("int", 0, "live", None),               # (unset: off)
    "RS_HIP_CHAIN_DEBUG_NO_SELFCHECK": ("flag", 0, "live", None),
    "RS_HIP_DEBUG_TOTALS": ("flag", 0, "live", None),
    "RS_HIP_SCORE_HIST": ("flag", 0, "live", None),
    "RS_HIP_SCHEDULE": ("word", 0, "live", None),
    # rs_dropin.cpp
    "RS_DROPIN_FULL_HASH": ("flag", 0, "first", None),
    "RS_DROPIN_FULL_HASH_BELOW": ("i64", 4 << 20, "first", None),
    "RS_DROPIN_FULL_HASH_SMALL": ("i64", 64 << 10, "first", None),
    "RS_DROPIN_HOST_QUERIES": ("i64", 4, "live", None),
    "RS_DROPIN_INIT_WITHOUT_DEVICE": ("flag", 0, "live", None),
    "RS_DROPIN_STATS": ("flag", 0, "boot", None),
}

# std::max( lo, value of the text ) around the parent's read: the least a SET name gives
AT_LEAST = {"RS_HIP_PROF_EVERY": 1, "RS_HIP_CHAIN_REFRESH": 0, "RS_HIP_CHAIN_DEBUG": 1}

# what the parent's setters stored of an argument >= 0 (the others: the argument as it is)
STORED = {
    "rs_hip_icp_exact_centroids": lambda v: 1 if v > 2 else v,
    "rs_hip_icp_early_plain": lambda v: 1 if v else 0,
    "rs_hip_icp_plain_from_records": lambda v: 1 if v else 0,
    "rs_hip_icp_update_fenced": lambda v: 1 if v else 0,
}
