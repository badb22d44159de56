// Every environment switch of librescan_hip.so and librescan_dropin.so, in one table: its name, how its value is parsed, its default,
// WHEN it is read, the C setter that changes it afterwards (include/rescan_hip.h), and what it is for.  Host only, plain C++17: the
// .hip units and rs_dropin.cpp (its own library, built by g++) include it, and nothing else under csrc/ reads the environment.
//
//   value kinds   FLAG   set at all, whatever the text (RS_HIP_NO_WARM=0 still turns warm starts off)
//                 INT / I64 / FLOAT / DOUBLE   atoi / atoll / (float)atof / atof of the text
//                 WORD   a text the reader interprets (sw_word); as a number: 1 when set
//   read classes  BOOT   once, when the library is loaded, into an atomic; the row's setter (if it has one) returns the previous value and stores a new one
//                 FIRST  latched by the first read: setting the name later in the same process changes nothing
//                 LIVE   from the environment whenever asked.  An entry point asks once per call and carries the answer (tests switch these)
//   stored as     what a setter keeps of its argument: ASIS, ONOFF (0 / 1), MODE (a value above 2 is 1)
//   at least      the smallest value a SET name can give (NO_MIN: none); the default is not clamped
//
// NOT here, because they are compile-time knobs (-D flags of tools/variant.sh): RS_DBG, RS_TAIL_DBG, RS_FAITH_TIMING, RS_FAITH_SPLIT,
// RS_PLAIN_XCD, RS_PLAIN_MAX_BLOCKS, CH_BUDGET, CH_ITEMS, RS_XCD_MAP, RS_XCD_CHUNK_LOG2, RS_XCD_CHUNK_WARM_LOG2, RS_ICP_CULL.  RS_HIP_LIB (which build the Python binding loads) and RS_BENCH_*
// belong to rescan_amd/capi.py and bench.py.
#pragma once

#include <atomic>
#include <cstdlib>
#include <cstring>
#include <mutex>

namespace rs {

#define SW_NO_MIN -1e300
//     id                        name                                 kind    default   class  setter                              stored  at least   meaning
#define RS_SWITCHES( X ) \
  /* ---- the ICP estimators (rs_api.hip: icp_choose) ---- */ \
  X( REF_ORDER_BELOW,          "RS_HIP_REF_ORDER_BELOW",            INT,    16384,    BOOT,  "rs_hip_icp_reference_order_below", ASIS,   SW_NO_MIN, "sources up to this many points: the reference's own summation order, its bits" ) \
  X( REPLAY_BELOW,             "RS_HIP_REPLAY_BELOW",               INT,    0,        BOOT,  "rs_hip_icp_replay_below",          ASIS,   SW_NO_MIN, "above that, up to this many points: the same bits summed in parallel (0: never)" ) \
  X( LANE_CHAINS_BELOW,        "RS_HIP_LANE_CHAINS_BELOW",          INT,    65536,    BOOT,  "rs_hip_icp_lane_chains_below",     ASIS,   SW_NO_MIN, "above those, up to this many points: the centroid chains by one wave each; beyond: spread over the chip" ) \
  X( EXACT_CENTROIDS,          "RS_HIP_EXACT_CENTROIDS",            INT,    1,        BOOT,  "rs_hip_icp_exact_centroids",       MODE,   SW_NO_MIN, "0: plain fp64 moments, 1: the reference's centroid chains, 2: those sums from the searches' records" ) \
  X( CHAINS_RETRY_AFTER,       "RS_HIP_CHAINS_RETRY_AFTER",         INT,    15,       BOOT,  "rs_hip_icp_chains_retry_after",    ASIS,   SW_NO_MIN, "calls a source skips the grid chains for after they gave one of its problems up" ) \
  X( FAITH_GUESS,              "RS_HIP_FAITH_GUESS",                INT,    1000,     BOOT,  "rs_hip_icp_faith_guess",           ASIS,   SW_NO_MIN, "the sequential estimator's guessed cut, per mille (0: three passes)" ) \
  X( STOP_GUARD,               "RS_HIP_STOP_GUARD",                 FLOAT,  1.5e-6,   BOOT,  "rs_hip_icp_stop_guard",            ASIS,   SW_NO_MIN, "a stop test decided within this of its threshold is run again in the reference's order (0: off)" ) \
  X( EARLY_PLAIN,              "RS_HIP_EARLY_PLAIN",                INT,    1,        BOOT,  "rs_hip_icp_early_plain",           ONOFF,  SW_NO_MIN, "plain early iterations of scan-sized sources (0: chains in every iteration)" ) \
  X( EARLY_TAIL,               "RS_HIP_EARLY_TAIL",                 INT,    0,        FIRST, "",                                 ASIS,   SW_NO_MIN, "chain iterations kept at the end of a call with plain early ones (0: two or three)" ) \
  X( PLAIN_RECORDS,            "RS_HIP_PLAIN_RECORDS",              INT,    0,        BOOT,  "rs_hip_icp_plain_from_records",    ONOFF,  SW_NO_MIN, "1: plain iterations from the searches' 48-byte records again" ) \
  X( UPDATE_FENCED,            "RS_HIP_UPDATE_FENCED",              INT,    0,        BOOT,  "rs_hip_icp_update_fenced",         ONOFF,  SW_NO_MIN, "1: k_icp_update_wide hands its sums over by two full fences again (the same bits)" ) \
  X( CHAIN_REFRESH,            "RS_HIP_CHAIN_REFRESH",              INT,    0,        FIRST, "",                                 ASIS,   0,         "re-guess the grid chains' binades in every k-th iteration (0: in the first only)" ) \
  X( ICP_CHUNK,                "RS_HIP_ICP_CHUNK",                  INT,    4,        FIRST, "",                                 ASIS,   SW_NO_MIN, "iterations enqueued between two looks at the loop state" ) \
  X( ICP_BATCH_BYTES,          "RS_HIP_ICP_BATCH_BYTES",            DOUBLE, 4e9,      FIRST, "",                                 ASIS,   SW_NO_MIN, "bytes of per-point records a slice of a batch of scan-sized problems may keep" ) \
  /* ---- the ICP searches ---- */ \
  X( NO_WARM,                  "RS_HIP_NO_WARM",                    FLAG,   0,        LIVE,  "",                                 ASIS,   SW_NO_MIN, "no search starts from the match of the iteration before" ) \
  X( NO_SEED,                  "RS_HIP_NO_SEED",                    FLAG,   0,        LIVE,  "",                                 ASIS,   SW_NO_MIN, "no seeding of a tile's search radius" ) \
  X( NO_BY_ROWS,               "RS_HIP_NO_BY_ROWS",                 FLAG,   0,        LIVE,  "",                                 ASIS,   SW_NO_MIN, "the cooperative kernel takes cells one by one instead of by rows" ) \
  X( NO_BOUNDED_ONLY,          "RS_HIP_NO_BOUNDED_ONLY",            FLAG,   0,        LIVE,  "",                                 ASIS,   SW_NO_MIN, "settled lanes keep streaming candidates" ) \
  X( NO_CERT,                  "RS_HIP_NO_CERT",                    FLAG,   0,        LIVE,  "",                                 ASIS,   SW_NO_MIN, "no certificates (searches skipped because the match cannot have changed)" ) \
  X( NO_RANK_CERT,             "RS_HIP_NO_RANK_CERT",               FLAG,   0,        LIVE,  "",                                 ASIS,   SW_NO_MIN, "certificates without the rank slack" ) \
  X( NO_LPT,                   "RS_HIP_NO_LPT",                     FLAG,   0,        LIVE,  "",                                 ASIS,   SW_NO_MIN, "slow tiles are not launched first" ) \
  X( SOLO_STAGES,              "RS_HIP_SOLO_STAGES",                INT,    -1,       FIRST, "",                                 ASIS,   SW_NO_MIN, "candidates a lone wave streams before its tile is handed off (-1: by launch size)" ) \
  X( HANDOFF_K,                "RS_HIP_HANDOFF_K",                  INT,    -1,       FIRST, "",                                 ASIS,   SW_NO_MIN, "the shell after which an unsettled tile is handed off whatever it streamed (-1: 1)" ) \
  X( HEAVY_STREAMED,           "RS_HIP_HEAVY_STREAMED",             INT,    400,      FIRST, "",                                 ASIS,   SW_NO_MIN, "slow-tile list: candidates streamed from which a tile counts as slow" ) \
  X( HEAVY_HANDOFF,            "RS_HIP_HEAVY_HANDOFF",              INT,    600,      FIRST, "",                                 ASIS,   SW_NO_MIN, "slow-tile list: the same for a tile that was handed off" ) \
  X( HEAVY_TOTAL,              "RS_HIP_HEAVY_TOTAL",                INT,    400,      FIRST, "",                                 ASIS,   SW_NO_MIN, "slow-tile list: its length limit per problem" ) \
  X( COOP_ALL_BELOW,           "RS_HIP_COOP_ALL_BELOW",             I64,    4096,     FIRST, "",                                 ASIS,   SW_NO_MIN, "launches of up to this many tiles go straight to the cooperative kernel" ) \
  X( COOP_WAVES,               "RS_HIP_COOP_WAVES",                 INT,    0,        FIRST, "",                                 ASIS,   SW_NO_MIN, "waves per queued tile in the cooperative kernel (0: by queue length)" ) \
  /* ---- clouds ---- */ \
  X( TILE_EXTENT_MAX,          "RS_HIP_TILE_EXTENT_MAX",            FLOAT,  0.3,      FIRST, "",                                 ASIS,   SW_NO_MIN, "largest extent of a query tile, metres" ) \
  X( AUTO_CELL_SCALE,          "RS_HIP_AUTO_CELL_SCALE",            FLOAT,  1.0,      FIRST, "",                                 ASIS,   SW_NO_MIN, "factor on the cell size derived from a cloud's density" ) \
  /* ---- alignment scores ---- */ \
  X( SCORE_SCENE,              "RS_HIP_SCORE_SCENE",                INT,    1,        FIRST, "",                                 ASIS,   SW_NO_MIN, "0: object tiles only, never the scene-space route" ) \
  X( SCORE_SCENE_MIN,          "RS_HIP_SCORE_SCENE_MIN",            I64,    65536,    BOOT,  "rs_hip_score_scene_space_from",    ASIS,   SW_NO_MIN, "queries (poses x points) from which a batch takes the scene-space route" ) \
  X( SCORE_SCENE_DENSITY,      "RS_HIP_SCORE_SCENE_DENSITY",        DOUBLE, 128.0,    FIRST, "",                                 ASIS,   SW_NO_MIN, "... and queries per lattice block it needs for that" ) \
  X( SCORE_PARENT,             "RS_HIP_SCORE_PARENT",               FLOAT,  1.0,      FIRST, "",                                 ASIS,   SW_NO_MIN, "scene-space route: edge of a parent block / radius" ) \
  X( SCORE_NBIN,               "RS_HIP_SCORE_NBIN",                 INT,    1,        FIRST, "",                                 ASIS,   SW_NO_MIN, "scene-space route: 0 keys without the normal bin" ) \
  X( SCORE_CULL,               "RS_HIP_SCORE_CULL",                 INT,    1,        FIRST, "",                                 ASIS,   SW_NO_MIN, "scene-space route: 0 keeps queries outside the scene's box" ) \
  X( SCORE_COUNTING,           "RS_HIP_SCORE_COUNTING",             INT,    22,       FIRST, "",                                 ASIS,   SW_NO_MIN, "scene-space route: key bits up to which the sort is a counting sort (0: the radix sort)" ) \
  /* ---- full-rows radius search ---- */ \
  X( ROWS_TILED_FROM,          "RS_HIP_ROWS_TILED_FROM",            I64,    4096,     LIVE,  "",                                 ASIS,   SW_NO_MIN, "short rows (k < 16) of at least this many queries take the tiled kernel" ) \
  X( NO_ROWS_WAVE,             "RS_HIP_NO_ROWS_WAVE",               FLAG,   0,        LIVE,  "",                                 ASIS,   SW_NO_MIN, "never one wave per query: every call takes the tiled kernel" ) \
  X( ROWS_ZERO_COPY_BELOW,     "RS_HIP_ROWS_ZERO_COPY_BELOW",       I64,    262144,   FIRST, "",                                 ASIS,   SW_NO_MIN, "result bytes up to which the kernel writes straight into pinned host memory" ) \
  X( ROWS_POLL,                "RS_HIP_ROWS_POLL",                  FLAG,   0,        FIRST, "",                                 ASIS,   SW_NO_MIN, "the host polls the counts instead of synchronising (not safe: kept for measurements)" ) \
  /* ---- the runtime, profiling, diagnostics ---- */ \
  X( SCHEDULE,                 "RS_HIP_SCHEDULE",                   WORD,   0,        LIVE,  "",                                 ASIS,   SW_NO_MIN, "spin: completion waits busy-wait (read by rs_hip_init)" ) \
  X( PROF_EVERY,               "RS_HIP_PROF_EVERY",                 INT,    1,        FIRST, "",                                 ASIS,   1,         "ICP calls per one that carries profile events" ) \
  X( DEBUG,                    "RS_HIP_DEBUG",                      FLAG,   0,        LIVE,  "",                                 ASIS,   SW_NO_MIN, "one ICP iteration per chunk, its counts on stderr" ) \
  X( DEBUG_CYCLES,             "RS_HIP_DEBUG_CYCLES",               FLAG,   0,        LIVE,  "",                                 ASIS,   SW_NO_MIN, "... with device timers per tile (diagnostic build, -DRS_DBG=1)" ) \
  X( DEBUG_TOTALS,             "RS_HIP_DEBUG_TOTALS",               FLAG,   0,        LIVE,  "",                                 ASIS,   SW_NO_MIN, "the last iteration's seven centroid sums on stderr" ) \
  X( LANE_DEBUG,               "RS_HIP_LANE_DEBUG",                 FLAG,   0,        LIVE,  "",                                 ASIS,   SW_NO_MIN, "the lane chains account for their walks" ) \
  X( CHAIN_DEBUG,              "RS_HIP_CHAIN_DEBUG",                INT,    0,        LIVE,  "",                                 ASIS,   1,         "the grid chains report their walks, each repeated this many times" ) \
  X( CHAIN_DEBUG_NO_SELFCHECK, "RS_HIP_CHAIN_DEBUG_NO_SELFCHECK",   FLAG,   0,        LIVE,  "",                                 ASIS,   SW_NO_MIN, "... without redoing every step the slow way" ) \
  X( SCORE_HIST,               "RS_HIP_SCORE_HIST",                 FLAG,   0,        LIVE,  "",                                 ASIS,   SW_NO_MIN, "histogram of the score kernel's candidates per query (diagnostic build)" ) \
  /* ---- librescan_dropin.so (rs_dropin.cpp) ---- */ \
  X( DROPIN_HOST_QUERIES,      "RS_DROPIN_HOST_QUERIES",            I64,    4,        LIVE,  "",                                 ASIS,   SW_NO_MIN, "searches of up to this many queries are answered from the grid's host copy" ) \
  X( DROPIN_FULL_HASH,         "RS_DROPIN_FULL_HASH",               FLAG,   0,        FIRST, "",                                 ASIS,   SW_NO_MIN, "the upload cache hashes every array whole on every call" ) \
  X( DROPIN_FULL_HASH_BELOW,   "RS_DROPIN_FULL_HASH_BELOW",         I64,    4194304,  FIRST, "",                                 ASIS,   SW_NO_MIN, "arrays up to this many bytes are keyed by their full hash or a strided one, larger ones by a sample" ) \
  X( DROPIN_FULL_HASH_SMALL,   "RS_DROPIN_FULL_HASH_SMALL",         I64,    65536,    FIRST, "",                                 ASIS,   SW_NO_MIN, "... and up to this many bytes always by their full hash" ) \
  X( DROPIN_STATS,             "RS_DROPIN_STATS",                   FLAG,   0,        BOOT,  "",                                 ASIS,   SW_NO_MIN, "calls and seconds per entry point and route, on stderr when the process ends" ) \
  X( DROPIN_INIT_WITHOUT_DEVICE, "RS_DROPIN_INIT_WITHOUT_DEVICE",   FLAG,   0,        LIVE,  "",                                 ASIS,   SW_NO_MIN, "msh_hash_grid_init_3d builds its host index without a device (tests)" )

enum SwKind { SW_FLAG, SW_INT, SW_I64, SW_FLOAT, SW_DOUBLE, SW_WORD };
enum SwClass { SW_BOOT, SW_FIRST, SW_LIVE };
enum SwStored { SW_ASIS, SW_ONOFF, SW_MODE };
enum SwId
{
#define X( id, name, kind, def, cls, setter, stored, lo, meaning ) SW_##id,
  RS_SWITCHES( X )
#undef X
  SW_COUNT
};
struct SwRow { const char* name; SwKind kind; double def; SwClass cls; const char* setter; SwStored stored; double lo; const char* meaning; };
inline constexpr SwRow SW_ROWS[SW_COUNT] = {
#define X( id, name, kind, def, cls, setter, stored, lo, meaning ) { name, SW_##kind, def, SW_##cls, setter, SW_##stored, lo, meaning },
  RS_SWITCHES( X )
#undef X
};

// a switch's value: integer kinds (and flags: 0 / 1) in i and d, FLOAT and DOUBLE in d only
struct SwVal { long long i; double d; };

inline SwVal sw_from_env( SwId id )
{
  const SwRow& r = SW_ROWS[id];
  const char* s = getenv( r.name );
  SwVal v{ (long long)r.def, r.kind == SW_FLOAT ? (double)(float)r.def : r.def };      // (0.3 -> 0.3f: the nearest float either way)
  switch( r.kind )
  {
  case SW_FLAG: case SW_WORD: v.i = s ? 1 : 0; break;
  case SW_INT:    if( s ) v.i = atoi( s ); break;
  case SW_I64:    if( s ) v.i = atoll( s ); break;
  case SW_FLOAT:  if( s ) v.d = (double)(float)atof( s ); break;
  case SW_DOUBLE: if( s ) v.d = atof( s ); break;
  }
  if( r.kind == SW_FLOAT || r.kind == SW_DOUBLE ) { if( s && v.d < r.lo ) v.d = r.lo; v.i = 0; }
  else { if( s && (double)v.i < r.lo ) v.i = (long long)r.lo; v.d = (double)v.i; }
  return v;
}

// What BOOT and FIRST rows hold (one per process and library: the units of librescan_hip.so share it).
struct SwTable
{
  struct Slot { std::atomic<long long> i{ 0 }; std::atomic<double> d{ 0.0 }; std::once_flag first; };
  Slot slot[SW_COUNT];
  void store( SwId id, SwVal v ) { slot[id].i.store( v.i ); slot[id].d.store( v.d ); }
  SwTable() { for( int k = 0; k < SW_COUNT; ++k ) if( SW_ROWS[k].cls == SW_BOOT ) store( (SwId)k, sw_from_env( (SwId)k ) ); }
};
inline SwTable g_switches;

// the value the library uses now
inline SwVal sw_value( SwId id )
{
  if( SW_ROWS[id].cls == SW_LIVE ) return sw_from_env( id );
  SwTable::Slot& s = g_switches.slot[id];
  if( SW_ROWS[id].cls == SW_FIRST ) std::call_once( s.first, [id] { g_switches.store( id, sw_from_env( id ) ); } );
  return { s.i.load(), s.d.load() };
}
// one accessor per kind
inline bool        sw_flag( SwId id )   { return sw_value( id ).i != 0; }
inline int         sw_int( SwId id )    { return (int)sw_value( id ).i; }
inline long long   sw_i64( SwId id )    { return sw_value( id ).i; }
inline float       sw_float( SwId id )  { return (float)sw_value( id ).d; }
inline double      sw_double( SwId id ) { return sw_value( id ).d; }
inline const char* sw_word( SwId id )   { return getenv( SW_ROWS[id].name ); }      // (WORD rows are LIVE)

// The body of every setter of a BOOT row: a negative argument only reads; returns the previous value.
template <class T> inline T sw_set( SwId id, T v )
{
  const SwRow& r = SW_ROWS[id];
  const SwVal prev = sw_value( id );
  if( v >= (T)0 )
  {
    if( r.stored == SW_ONOFF ) v = v ? (T)1 : (T)0;
    if( r.stored == SW_MODE && v > (T)2 ) v = (T)1;
    g_switches.store( id, { r.kind == SW_FLOAT || r.kind == SW_DOUBLE ? 0 : (long long)v, (double)v } );
  }
  return r.kind == SW_FLOAT || r.kind == SW_DOUBLE ? (T)prev.d : (T)prev.i;
}

inline int sw_find( const char* name )
{
  for( int k = 0; name && k < SW_COUNT; ++k ) if( !std::strcmp( name, SW_ROWS[k].name ) ) return k;
  return -1;
}

} // namespace rs
