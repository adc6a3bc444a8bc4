// fac_internal.h — host/device data layout of the MI355X fuzzy Aho–Corasick engine.
//
// The reference keeps a `Vec<Node>` of 112-byte nodes, each owning two heap `Vec`s and a
// hash map (structs.rs:249-281). On MI355X the automaton is flattened into structure-of-arrays
// tables that stay L2-resident (≈1-5 MB at 10K patterns) and are read with wave-uniform loads:
//
//   DevNode[N]   32 B  prune_len, prune_len_over_weight, edge_begin, degree | has-output, and the
//                      node's single-ASCII-byte edge map (structs.rs:471-493): one load per pop
//   out_range[N]  8 B  output range (read on emission only); node_pidx[N] 4 B pattern_index
//   DevEdge[E]    8 B  first code point | target node + (child-has-output, single-byte) flag bits
//   sb_edge[E]   16 B  sb_bits of each edge's child (one parent edge per node: loads in parallel
//                      with the edge record instead of after it)
//   out_pat[O]    4 B  output pattern ids (own + fail-merged, builder.rs:235,264-268)
//   DevPattern[P]32 B  grapheme_len as f32, weight, per-pattern limits
//   sim_ascii  64 KiB  128x128 f32 similarity table (structs.rs:36-48) + sorted non-ASCII pairs
#pragma once

#include <hip/hip_runtime.h>

#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <unordered_map>
#include <string>
#include <vector>

#include "../../include/fac.h"

namespace fac {

// ---------------------------------------------------------------- unicode.cpp
uint32_t utf8_decode(const uint8_t* s, uint64_t n, uint64_t& i);
bool utf8_valid(const uint8_t* s, uint64_t n, bool* ascii = nullptr);  // ascii: also whether every byte < 0x80
uint64_t utf8_valid_prefix(const uint8_t* s, uint64_t n);
void segment_graphemes(const uint8_t* s, uint64_t n, std::vector<uint64_t>& starts);
int lower_full(uint32_t cp, uint32_t out[3]);
void fold_grapheme(const uint8_t* s, uint64_t b, uint64_t e, bool ci, std::u32string& out);
uint32_t fold_first_char(const uint8_t* s, uint64_t b, uint64_t e, bool ci);
// The whole-token rule (fac.h fac_batch_require_boundaries). boundary_class: bit 0 alphanumeric
// (Rust's char::is_alphanumeric), bit 1 transparent (General_Category M* and not alphanumeric); 0 for
// surrogates and values above U+10FFFF. boundary_ok: whether the sides `sides` of [start, end) are
// boundaries of the valid UTF-8 text s[0, n); start <= end <= n, both on character boundaries.
constexpr uint32_t kBoundaryMaxSkip = 32;  // transparent code points the start side walks over
uint32_t boundary_class(uint32_t cp);
bool boundary_ok(const uint8_t* s, uint64_t n, uint64_t start, uint64_t end, int sides);
// The rule for a stream window (fac.h fac_stream_open_opts): s[0, n) is the window's text and
// before[0, before_len) the stream's text just before it; the start side's walk goes on into the
// context, and its front is the stream's start only when !more_before. 1 kept, 0 dropped, -1 when
// the walk reaches the front of a context that has text before it undecided (never with
// before_len >= kBoundaryCarry: the walk reads at most kBoundaryMaxSkip code points of 4 bytes).
constexpr uint32_t kBoundaryCarry = 4 * kBoundaryMaxSkip;
int boundary_ok_after(const uint8_t* before, uint64_t before_len, bool more_before, const uint8_t* s, uint64_t n,
                      uint64_t start, uint64_t end, int sides);

// ---------------------------------------------------------------- device layout
constexpr uint32_t EDGE_SINGLE_BYTE = 1u << 31;
constexpr uint32_t EDGE_CHILD_OUTPUT = 1u << 30;
constexpr uint32_t EDGE_NEXT_MASK = (1u << 30) - 1;
constexpr uint32_t CHILD26_MASK = (1u << 26) - 1;  // node ids are < 2^26 (builder limit)

// goto table entry: kv = GT_VALID | kind << 47 | node << 21 | char; val by kind:
//   GT_GOTO: first edge of `node` whose first char is `char`: child | edge index << 32 | own-single-byte << 40
//   GT_SB:   bit i = child of edge i has a single-byte edge labelled `char` (char < 128)
constexpr uint64_t GT_VALID = 1ull << 63;
constexpr uint64_t GT_GOTO = 0, GT_SB = 1ull << 47;
// 2-choice cuckoo table of 16 B entries {kv, val}: a key lives at gt_slot(kv, seed1) or
// gt_slot(kv, seed2); lookups read both slots, no probing
__host__ __device__ inline uint32_t gt_mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7FEB352Du;
  x ^= x >> 15;
  x *= 0x846CA68Bu;
  x ^= x >> 16;
  return x;
}
// both cuckoo slots from one 32-bit hash: a base hash of (node, char) shared by the GOTO and SB
// keys of that pair (the SB hash is an affine step away), low bits and the 16-bit rotation
__host__ __device__ inline uint32_t gt_base(uint32_t node, uint32_t ch, uint64_t seed) {
  return gt_mix32(((node << 21) | ch) ^ gt_mix32((node >> 11) ^ (uint32_t)seed));
}
// char filters (Engine::aux, GOTO values bits 48-63): one bit per hashed code point, a clear bit
// proves the (node, char) lookup would miss
__host__ __device__ inline uint32_t ch_filt_bit(uint32_t c) { return (c * 0x9E3779B1u) >> 27; }
__host__ __device__ inline uint32_t filt_fold16(uint32_t f) { return (f | (f >> 16)) & 0xFFFFu; }
__host__ __device__ inline uint32_t gt_kind_hash(uint32_t base, bool sb) {
  return sb ? base * 0x9E3779B1u + 0x7F4A7C15u : base;
}
__host__ __device__ inline void gt_slots_h(uint32_t h, uint32_t mask, uint32_t& s1, uint32_t& s2) {
  s1 = h & mask;
  s2 = ((h >> 16) | (h << 16)) & mask;
}
__host__ __device__ inline void gt_slots(uint64_t kv, uint64_t seed, uint32_t mask, uint32_t& s1, uint32_t& s2) {
  const uint32_t node = (uint32_t)((kv >> 21) & ((1u << 26) - 1)), ch = (uint32_t)(kv & ((1u << 21) - 1));
  gt_slots_h(gt_kind_hash(gt_base(node, ch, seed), (kv & GT_SB) != 0), mask, s1, s2);
}
constexpr int32_t LIM_NONE = -1;

struct U32StrHash {
  size_t operator()(const std::u32string& s) const {
    uint64_t h = 1469598103934665603ull;
    for (char32_t c : s) h = (h ^ (uint64_t)c) * 1099511628211ull;
    return (size_t)h;
  }
};

// host-side node (builder, host bookkeeping)
struct HostNode {
  float prune_len;
  float prune_lw;
  uint32_t edge_begin, edge_end;
  uint32_t out_begin, out_end;
  int32_t pidx;  // pattern_index (first pattern touching the node), -1 = None
};

// device node: one 32 B load gives everything a pop needs
constexpr uint32_t NODE_HAS_OUT = 1u << 31;
constexpr uint32_t NODE_DUP_CH = 1u << 30;     // two of the node's edges share a first char
constexpr uint32_t NODE_ASCII_EDGE = 1u << 29; // some edge's first char is ASCII
constexpr uint32_t NODE_DEG_MASK = (1u << 24) - 1;
struct alignas(16) DevNode {
  float prune_len;
  float prune_lw;
  uint32_t edge_begin;
  uint32_t degf;  // degree | NODE_HAS_OUT
  uint4 sb;       // 128-bit map of the node's single-ASCII-byte edge chars (structs.rs:471-493)
};
static_assert(sizeof(DevNode) == 32, "DevNode layout");

struct DevEdge {
  uint32_t ch;    // first char of the folded grapheme
  uint32_t next;  // target | EDGE_CHILD_OUTPUT | EDGE_SINGLE_BYTE
};

struct DevLimits {
  int32_t ins, del, sub, swp, edits;  // LIM_NONE = None
};

struct alignas(16) DevPattern {
  float glen;    // grapheme_len as f32 (search.rs:696)
  float weight;  // Pattern::weight
  int32_t has_limits;
  DevLimits lim;
};
static_assert(sizeof(DevPattern) == 32, "DevPattern layout");

// Dedup entry / queued state, 16 B. j and matched_end are stored relative to the window start
// (matched_start == start for every state of a window).
struct alignas(16) KState {
  uint32_t node;
  uint32_t jm;     // j_rel | me_rel << 16
  float pen;
  uint32_t packed;  // ins | del << 8 | sub << 16 | swp << 24 (structs.rs:173-176)
};

// A (sub)haystack searched as if it were the whole `haystack` argument of search_raw: the prefilter
// re-searches merged windows as independent slices (prefilter.rs:346-350), shards of one haystack
// keep the global length but only own a window range, and batches hold several haystacks.
struct SegDesc {
  uint64_t text_base;  // ascii: byte index of local grapheme 0 in `utf8`; unicode: grapheme index
  uint64_t n;          // text_len of the (sub)haystack (search.rs:440)
  uint64_t avail;      // local graphemes resident (>= every j the windows can reach, else ERR_HALO)
  uint64_t hay_len;    // byte length of the (sub)haystack (end_byte when me >= n, search.rs:672-676)
  uint64_t byte_base;  // global byte offset of local byte 0 (added to every output offset)
  uint64_t w_begin, w_end;  // local start windows to search
  uint32_t ascii;      // 1: grapheme == byte (AsciiGraphemes), 0: Unicode graphemes
  uint32_t pad;
};

// one prefix-cache level: open-addressing table of key hashes -> entry -> snapshot
struct RcTable {
  uint32_t k;                        // key chars
  uint32_t mask;                     // slots - 1
  const unsigned long long* keys;    // 0 = empty slot
  const uint32_t* val;               // entry of each slot (EMPTY: not cached)
  const uint32_t* off;               // snapshot offset of each entry (pool words)
  const uint32_t* count;             // queued states of each entry (EMPTY: not cached)
  // lookup table of the built entries (rc_publish_kernel): 32-byte slots {exact key: the k chars as
  // 16-bit units, padded with 0xFFFF; snapshot offset, head, queue length | best entries << 16,
  // occupied | dedup entries << 22 | pops}
  const uint4* ct;
  uint32_t ct_mask;                  // lookup slots - 1
};

constexpr int N_COUNTERS = 12;  // SearchParams::counters (8: lane-searched windows, 9: lane work counter, 10: lookup
                                // regions, 11: snapshots a cache build kept)
constexpr int kRcLevels = 5;   // prefix-cache levels: level 0 (under level 1), level 1, up to 3 sampled levels

struct SearchParams {
  // automaton
  const DevNode* nodes;
  const DevEdge* edges;
  const uint32_t* out_pat;
  const uint2* out_range;
  const int32_t* node_pidx;
  // O(1) expansion tables (builder.cpp "goto table"): (node, char) -> first edge / child maps
  const uint4* gt;            // cuckoo slots {kv lo, kv hi, val lo, val hi}
  uint32_t gt_mask;           // slot count - 1
  unsigned long long gt_seed1, gt_seed2;
  int32_t gt_fast;            // similarity can never drop a substitution when p_sub <= remaining
  // per node {child-has-output mask lo, hi (degree <= 64), child char filter, grandchild single-byte
  // char filter}: the filters (bit ch_filt_bit(c)) gate goto-table lookups that would miss
  const uint4* aux;
  const uint4* sb_edge;
  const DevPattern* pats;
  const float* sim_ascii;
  const uint64_t* sim_keys;  // (a << 32 | b), sorted
  const float* sim_vals;
  uint32_t n_sim;
  // haystack storage
  const uint8_t* utf8;     // raw bytes (ascii segments read graphemes from here)
  const uint32_t* text32;  // folded first code point per grapheme (unicode segments)
  const uint64_t* off;     // global byte offset per grapheme (unicode segments)
  const SegDesc* segs;
  const uint64_t* seg_prefix;  // exclusive prefix of (w_end - w_begin), n_segs + 1 entries
  uint32_t n_segs;
  uint64_t total_windows;
  int32_t case_insensitive;
  // scoring
  float thr;
  float max_penalties;
  float p_ins, p_del, p_sub, p_swp;
  float min_sym;
  uint32_t mef;  // MAX_EDITS_FAST (1..6) or 255
  int32_t has_glim;
  DevLimits glim;
  int32_t has_pattern_limits;
  uint32_t beam;  // 0 = None
  int32_t window_skip;
  uint32_t first_bits[4], second_bits[4];
  // work distribution / outputs
  uint32_t chunk;
  uint32_t ecap;            // per-wave emission list capacity
  uint4* ebuf;              // per-wave emission scratch (slice = the wave's slot)
  // wave slots (bfs_window_body): a launch may have more workgroups than resident waves (the
  // one-chunk-per-workgroup level-1 build), so per-wave global scratch is indexed by a slot taken
  // from a free ring when the wave starts and returned when it ends (slot_ctr: taken, returned)
  unsigned int* slot_ring;
  unsigned int* slot_ctr;
  uint32_t n_slots;
  uint4* bsel;              // beamed engines: the beam selection's scratch (bsel_stride per slot). An HBM rung
  uint32_t bsel_stride;     // (bfs_window_kernel_hbm): each slot's dedup table, ring, then that scratch
  uint32_t sel_limit;       // select.rs partition rounds before median_of_medians (16; tests lower it)
  int32_t beam_canonical;   // diagnostics (FAC_BEAM_CANONICAL): rounds 1-2's canonical tie rule
  fac_match* out;
  uint64_t out_cap;
  uint64_t out_shift;       // added to every record's start/end (global byte of a shard's byte 0)
  unsigned long long* counters;  // [0] matches, [1] states popped, [2] error flags, [3] spilled windows,
                                 // [4] pops replayed from snapshots, [5] windows resumed from a snapshot,
                                 // [6] of those, finished by the snapshot alone (empty queue),
                                 // [7] next window chunk (dynamic chunk hand-out)
  int32_t rc_lane_flush;         // resumed windows with an empty queue are flushed lane-parallel
  int32_t dyn_chunks;            // 1: chunks from the work counter; 0: static grid-stride
  uint32_t lane_popmax;           // lane_window_kernel: pops after which a window goes back to the wave kernel
  uint32_t live_nqmax;            // bfs_window_kernel_live: windows resuming with a longer queue go straight to the
                                  // exact variant (0: none)
  int32_t lane_debug;             // lane_window_kernel: diagnostics counters (FAC_RC_DEBUG)
  // window list mode (re-run of spilled windows) and the spill list of capacity overflows
  const uint64_t* win_list;  // null: virtual windows 0..total_windows; else list of virtual ids
  uint64_t* spill;           // virtual ids of windows that overflowed this variant's LDS frontier
  uint64_t spill_cap;
  // auto-beam pass 1 (search.rs:1096-1103): per window queue.len() under exact dedup
  uint32_t* win_counts;  // null: not recorded
  int32_t exact_dedup;   // dedup must be exact (beam, or counting for auto-beam)
  int32_t dup_cut;       // diagnostics (FAC_DUP_CUT=1): cut a batch at an in-batch duplicate instead of resolving it
  // prefix cache (launch_pass): a state at j reads text[j] and text[j + 1], so the
  // pops before the first state with j >= rc_k - 1 depend only on the window's first rc_k chars;
  // windows sharing them resume from one snapshot (queue, dedup entries, best list, counters)
  // Two levels: short keys for every window, long keys for the frequent prefixes only; a lookup
  // takes the deepest hit (rc_tab[0] first). A level-2 build resumes its representatives from
  // level-1 snapshots.
  int32_t rc_mode;                  // 0 off, 1 use the cache, 2 build it (win_list = representatives)
  uint32_t rc_k;                    // key chars of the level being collected / built (2..8)
  uint32_t rc_ntab;                 // tables a lookup consults (0..kRcLevels), deepest first
  uint32_t rc_kstart;               // rc_lookup's first probe: the shallowest level with k >= this (0: the
                                    // shallowest level; a k no level has, 0xFFFFFFFF: the deepest level)
  uint4* rc_bhits;                  // cache build: each key's parent snapshot (rc_parent_kernel), as rc_hits
  uint32_t* rc_bpops;               // ... and its pops
  RcTable rc_tab[kRcLevels];
  uint32_t rc_vmax, rc_emax;        // dedup / best-list entries a snapshot may hold
  uint4* rc_pool;                   // snapshots: header x4, queue, dedup entries, best list
  unsigned long long rc_pool_cap;   // pool words (uint4)
  unsigned long long* rc_pool_used; // bump allocator
  uint32_t rc_pool_chunk;           // pool words a building wave takes at a time
  uint32_t rc_qcap;                 // main pass ring: snapshots with more queued states are not resumed
  uint4* rc_hits;                   // main pass: per window {offset | RC_DONE, head, tail, nv | ne << 16}
  uint32_t* rc_hit_pops;            // ... and the snapshot's pops
  // main pass: rc_hits / rc_hit_pops hold only the windows the lookups leave open, compacted per
  // region of RC_REGION windows (entries [r * RC_REGION, + rc_region_cnt[r])); rc_voff = the window
  // of each entry as its offset in the region
  uint32_t* rc_voff;
  uint32_t* rc_region_cnt;
  uint32_t* rc_off;                 // build: snapshot offset of each entry (pool words)
  uint32_t* rc_count;               // build: queued states of each entry (EMPTY: not cached)
  int32_t rc_keep_final;            // build: snapshot a key whose parent is final too (its level is
                                    // looked up without the parent's: level 1 over level 0)
  // multi-character mappings (search.rs:776-780, 883-922, 945-961; builder.rs:383-442). With
  // has_map, exact and swap transitions compare whole folded graphemes (ids, 0 = not in the
  // engine's grapheme dictionary): edge_gid per edge, text gids per grapheme (gid32 for Unicode
  // segments, ascii_gid[folded byte] for ASCII ones)
  int32_t has_map;
  const uint32_t* edge_gid;
  const uint32_t* gid32;
  const uint32_t* ascii_gid;  // 128 entries
  const uint2* map_range;     // per node [begin, end) into map_ent
  const uint4* map_ent;       // {hay begin (into map_hay), hay length, next node, penalty bits}
  const uint32_t* map_hay;    // haystack-side grapheme ids
  // key partition of the haystack's start windows (Haystack::kparts / kpart), last: fields added
  // in the middle moved every later kernel argument and changed the window kernels' allocation
  uint32_t kp_n, kp_r;
  // the key part's start windows, ascending (rc_count_kernel / rc_lookup_kernel walk them; the
  // lookup stores each open window as its list region's base + offset, so the searches' entry ->
  // window mapping needs no list)
  const uint64_t* kp_wlist;
  // dense start-level key bitmaps (rc_dense_*_kernel, search_kernels.hip): rank table, alphabet size,
  // "final without records" and "cached" bits over the keys of ranked characters; null: none
  const uint32_t* rc_dense;
  // diagnostics (FAC_RC_FULL_SWEEP=1): the build epilogue sweeps the dedup table for final keys too
  // and re-reads every slot in both writing passes (the epilogue before the single sweep; same pool)
  int32_t rc_full_sweep;
  // carry-over (RcStore): rc_carry_kernel ran ahead of this level's build, and the entries
  // whose rc_off is not RC_TOBUILD hold a snapshot of an earlier call (rc_parent_kernel and the build
  // skip them). Last, like the fields above.
  int32_t rc_carry;
};

constexpr unsigned ERR_QUEUE = 1u, ERR_VISITED = 2u, ERR_EMIT = 4u, ERR_HALO = 8u, ERR_OUT = 16u, ERR_SPILL = 32u;

// ---------------------------------------------------------------- engine
// The pre-filter's device tables for one set of edit budgets (prefilter_kernels.hip prefilter_windows):
// the packed full-scan words and the q-gram path's gram table, screening bitmap and pattern masks.
// Built on a call's first use and kept by the engine (they depend on the engine and ks alone).
struct PfTables {
  std::vector<uint32_t> ks;
  bool want_bytes = false;  // the key: built for a byte-reading scan (if the q-gram path takes every pattern),
  bool qgram_on = true;     // and the FAC_NO_QGRAM knob's state
  bool bytes = false;       // the grams keyed by case-folded bytes (else by symbol ids)
  uint32_t nw = 0, kmax = 0;  // packed full scan: automaton words, largest edit budget
  bool w32 = true;
  void *pmask = nullptr, *ptop = nullptr, *wk = nullptr;
  bool q = false;           // q-gram path in use
  uint32_t ts = 0, use3 = 0, use4 = 0, use5 = 0, kq = 0, mq = 0;
  size_t n_qpat = 0, n_grams = 0, n_keys = 0;
  void *tab = nullptr, *ent = nullptr, *qmask = nullptr, *qpm = nullptr, *qbits = nullptr;
  void* m16 = nullptr;      // every q-gram pattern m <= 16: 16-bit masks [pattern][rows] for LDS
  uint32_t m16_words = 0;
  ~PfTables() {
    for (void* p : {pmask, ptop, wk, tab, ent, qmask, qpm, qbits, m16})
      if (p) (void)hipFree(p);
  }
};

// A device lookup "folded grapheme -> id" (stage_kernels.hip): an open-addressing table over a hash
// of the grapheme's folded code points. A slot holds an entry's index + 1 (0: empty), an entry
// {hash, offset of its key in the pool, key length in code points, id}; the pool holds every key's
// code points. Keys have any length and ids are 32 bits: Engine::sym_tab holds the pre-filter's
// symbols, Engine::gid_tab the grapheme dictionary of an engine with mappings (Engine::gid_of).
struct GraphemeTable {
  uint32_t* d_slots = nullptr;
  uint4* d_ents = nullptr;
  uint32_t* d_pool = nullptr;
  uint32_t mask = 0;  // slots - 1
  uint32_t n_keys = 0, n_pool = 0;
};

// Engine-resident snapshot store: the snapshot pool and one exact-key directory
// per key length, kept from call to call, so that a level's build runs only for the keys no earlier
// call built. One call at a time uses it (mu, try-lock; a call that finds it taken runs with a pool
// from call scratch and no carry-over). Host state only here: device_state.cpp owns the allocations.
constexpr int kRcSigWords = 16;
constexpr uint32_t RC_TOBUILD = 0xFFFFFFFDu;  // rc_off of an entry rc_carry_kernel did not find
// a call goes direct with an unknown share up to this far (per mille) above the store's floor
// (FAC_RC_DIRECT_PM; the sweep is in DESIGN.md §6)
constexpr uint32_t kRcDirectPm = 20;
enum RcReset { kRcKeep = 0, kRcFresh, kRcSignature, kRcPool, kRcDirectory, kRcBusy, kRcOff, kRcGated };
const char* rc_reset_name(int r);
struct RcStoreDir {
  uint4* slots = nullptr;  // rc_publish_kernel's 32-byte slots
  uint32_t n_slots = 0;    // a power of two (0: none yet)
  uint64_t count = 0;      // keys inserted (host copy, read back at the end of each call)
  uint64_t peak = 0;       // the most it has held (sizes it when it is allocated again)
};
struct RcStore {
  std::mutex mu;
  bool valid = false;            // sig, the pool's contents and the directories belong together
  uint32_t sig[kRcSigWords] = {};
  uint4* pool = nullptr;
  uint64_t cap = 0;              // pool words allocated
  uint64_t used = 0;             // pool words used (host copy of dev[0])
  uint64_t last_call = 0;        // pool words the previous call appended
  int pending = kRcKeep;         // a reset the previous call asks of the next one (the pool ran out)
  // the gate for unlike text: a carrying call that found under a tenth of its entries sends the next
  // `sleep` calls past the store (1, 2, 4, .. 64 calls: `backoff`), and the store starts empty after them
  uint32_t sleep = 0, backoff = 0;
  RcStoreDir dir[9];             // by key length (2..8)
  uint64_t last_built[9] = {};   // entries the previous call built, by key length (sizes the waves' pool chunks)
  uint64_t carried[9] = {};      // entries the last call carried over, by key length
  // device words: [0] pool words used, [1 + k] entries carried at key length k (this call),
  // [10 + k] keys in directory k, [20] rc_store_sample_kernel's counts
  unsigned long long* dev = nullptr;
  static constexpr int kDevWords = 21;
  hipEvent_t last = nullptr;     // the previous user's last work on the store
  uint64_t calls = 0;
  // Direct calls: what the last full call left for a call that searches from the
  // directories alone. Reset with the directories (rc_store_prepare, rc_store_drop).
  uint32_t lv_k[kRcLevels] = {}; // that call's levels, deepest first (key lengths)
  uint32_t lv_n = 0;
  uint32_t kstart = 0;           // its SearchParams::rc_kstart
  uint64_t lv_knobs = 0;         // a hash of the level knobs it ran under (FAC_RC_K, FAC_RC_LEVELS, ...)
  int32_t floor_pm = -1;         // the unknown share (per mille of sampled windows) it left; < 0: none yet
  uint32_t* dense = nullptr;     // its dense start-level bitmaps (RC_DENSE_WORDS words, allocated on first use)
  bool has_dense = false;
  // the emptied-store gate: the last call that used the store started it empty (rc_store_emptied_gate)
  bool filled = false;
};
// what a call does with the store it has locked (no device work): kRcKeep carries over, every other
// value starts from an empty store (kRcFresh: it was empty already)
int rc_store_decide(const RcStore& s, const uint32_t sig[kRcSigWords], uint64_t want_cap, uint64_t cap_limit);
// directory k can take n more keys at a load of at most one half
bool rc_dir_fits(const RcStoreDir& d, uint64_t n);
int rc_store_prepare(RcStore& s, int decision, const uint32_t sig[kRcSigWords], uint64_t want_cap, hipStream_t st,
                     std::string& err);  // pool of want_cap words, empty directories
int rc_store_dir(RcStore& s, uint32_t k, uint64_t n_ent, hipStream_t st, std::string& err);  // directory k for n_ent more keys
// after the stream's sync: counts read back; carrying: the call carried over (the gate judges it);
// gate_min: calls with fewer entries are not judged
int rc_store_finish(RcStore& s, uint64_t cap_limit, bool carrying, uint64_t gate_min, std::string& err);
// the gate alone: the back-off after a carrying call with these totals (0: the store stays in use)
uint32_t rc_store_gate(uint64_t carried, uint64_t built, uint32_t backoff, uint64_t gate_min);
// the gate for a store that every call empties: the calls that go without the store, this one included,
// when `decision` (rc_store_decide) empties the store for its pool or a directory right after the call
// that filled it from empty (after_fill); 0: the rule does not apply and the call goes on as decided
uint32_t rc_store_emptied_gate(int decision, bool after_fill, uint32_t backoff);
// a call searches from the store's directories alone (no counts, selections or builds): unknown_pm of
// its `sampled` windows ended on a key no directory holds, against the share the last full call left
// (floor_pm, < 0: none) plus margin_pm; calls of fewer than min_windows windows never do
bool rc_direct_decide(uint32_t unknown_pm, int32_t floor_pm, uint32_t margin_pm, uint64_t sampled, uint64_t windows,
                      uint64_t min_windows);
int rc_store_dense(RcStore& s, size_t words, std::string& err);  // s.dense allocated (contents untouched)
void rc_store_drop(RcStore& s);  // frees everything (the caller holds mu)

struct Engine {
  int device = 0;
  hipStream_t stream = nullptr;
  // prefix cache: level-1 build beside the sampled-level counts (lowest priority; created with the
  // engine's tables; a streaming worker's ScratchSet has its own)
  hipStream_t aux_stream = nullptr;
  fac_config cfg{};
  bool case_insensitive = false;
  bool has_limits = false;
  DevLimits limits{LIM_NONE, LIM_NONE, LIM_NONE, LIM_NONE, LIM_NONE};
  bool has_pattern_limits = false;
  uint32_t max_edits_fast = 0;
  uint32_t mef = 255;
  uint64_t beam_width = 0;
  bool has_auto_beam = false;
  uint64_t ab_budget = 0, ab_width = 0;
  float p_ins, p_del, p_sub, p_swp, min_sym;
  // host tables
  std::vector<HostNode> nodes;
  std::vector<DevNode> dnodes;
  std::vector<uint2> out_range;
  std::vector<int32_t> node_pidx;
  std::vector<DevEdge> edges;
  std::vector<uint32_t> out_pat;
  std::vector<uint4> sb_bits;
  std::vector<uint4> sb_edge;
  std::vector<uint4> gt;  // goto table (cuckoo slots)
  uint32_t gt_mask = 0;
  uint64_t gt_seed1 = 0, gt_seed2 = 0;
  bool gt_fast = false;
  std::vector<uint4> aux;  // SearchParams::aux
  std::vector<uint32_t> pat_bytes;  // Pattern::len (bytes, structs.rs:628-630) for ranking
  std::vector<DevPattern> pats;
  std::vector<float> sim_ascii;
  std::vector<uint64_t> sim_keys;
  std::vector<float> sim_vals;
  uint32_t max_degree = 0;
  uint32_t max_degree_nonroot = 0;
  uint32_t max_glen = 0;
  uint64_t max_match_graphemes = 0;
  bool window_skip = false;
  uint32_t first_bits[4] = {0, 0, 0, 0}, second_bits[4] = {0, 0, 0, 0};
  // prefilter (prefilter.rs:69-93)
  bool bitap_ok = false;
  float edit_cost_mult = 0.f;
  uint8_t ascii_id[128] = {0};
  std::vector<std::pair<std::u32string, uint32_t>> symbol_ids;  // sorted by key
  // multi-character mappings (builder.rs:383-442); has_map = the precomputed table is non-empty
  bool has_map = false;
  std::unordered_map<std::u32string, uint32_t, U32StrHash> gid_of;  // folded grapheme -> id (1-based)
  std::vector<uint32_t> edge_gid;   // per edge
  uint32_t ascii_gid[128] = {0};    // id of each (folded) ASCII byte, 0 = none
  std::vector<uint2> map_range;     // per node
  std::vector<uint4> map_ent;
  std::vector<uint32_t> map_hay;
  uint32_t max_map = 0;             // most mapping transitions at one node (<= 64)
  uint32_t alphabet = 0;
  std::vector<uint32_t> bp_m;
  std::vector<float> bp_weight;
  std::vector<int64_t> bp_k_limit;  // -1 = None
  std::vector<uint64_t> bp_mask;    // P x (alphabet+1)
  // device copies
  DevNode* d_nodes = nullptr;
  DevEdge* d_edges = nullptr;
  uint32_t* d_out_pat = nullptr;
  uint2* d_out_range = nullptr;
  int32_t* d_pidx = nullptr;
  uint4* d_sb_edge = nullptr;
  uint4* d_gt = nullptr;
  uint4* d_aux = nullptr;
  uint32_t* d_pat_bytes = nullptr;
  DevPattern* d_pats = nullptr;
  float* d_sim_ascii = nullptr;
  uint64_t* d_sim_keys = nullptr;
  float* d_sim_vals = nullptr;
  uint8_t* d_ascii_id = nullptr;
  GraphemeTable sym_tab;  // symbol_ids on the device (bitap_ok engines; symbol_ids_device)
  GraphemeTable gid_tab;  // gid_of on the device (has_map engines; grapheme_ids_device)
  uint32_t* d_edge_gid = nullptr;
  uint32_t* d_ascii_gid = nullptr;
  uint2* d_map_range = nullptr;
  uint4* d_map_ent = nullptr;
  uint32_t* d_map_hay = nullptr;
  std::mutex mu;  // guards lazily grown scratch below
  // per-engine device scratch of the search launcher, reused across calls by whichever call holds
  // scratch_mu (a concurrent call on the same engine allocates its own)
  mutable std::mutex scratch_mu;
  mutable std::mutex pf_mu;  // guards pf_cache
  mutable std::vector<std::unique_ptr<PfTables>> pf_cache;
  static constexpr int kScratch = 64;
  mutable void* scratch_p[kScratch] = {};
  mutable size_t scratch_n[kScratch] = {};
  mutable RcStore rc_store;  // prefix-cache snapshots kept across calls
};

struct Haystack {
  bool ascii = true;
  uint64_t len = 0;  // bytes
  uint64_t n = 0;    // graphemes
  // shard of a larger haystack (fac_haystack_stage_shard): output offsets are shifted by `base`
  // (global byte of local byte 0); `open_end`: the text continues past the resident bytes, which
  // hold only the halo (j == n / end-of-text logic never applies); start windows [0, owned)
  uint64_t base = 0;
  bool open_end = false;
  uint64_t owned = UINT64_MAX;
  // key partition (fac_haystack_set_key_partition): only the start windows whose first two
  // characters hash to part (of parts) are searched -- a strong-scaling split of one haystack that
  // keeps every window of a prefix on one GPU, so each GPU's prefix cache covers whole keys
  uint32_t kparts = 1, kpart = 0;
  uint8_t* d_utf8 = nullptr;
  bool own_utf8 = true;          // false: the caller's device bytes (fac_haystack_stage_device)
  uint32_t* d_text32 = nullptr;  // Unicode only
  uint64_t* d_off = nullptr;     // Unicode only
  uint64_t off_cap = 0;          // entries d_off / d_text32 hold (kept when staged again)
  void* d_stage = nullptr;       // staging scratch (stage_device), kept when staged again
  size_t stage_cap = 0;
  // host copies, fetched from the device on first use (ensure_host): the UTF-8 bytes (shard
  // planning) and the grapheme byte starts (Unicode only)
  mutable std::vector<uint8_t> utf8;
  mutable std::vector<uint64_t> starts;
  mutable bool host_ready = false;
  mutable std::mutex host_mu;
  // grapheme ids (Unicode, engines with mappings): written by the device on the first search after
  // a staging (ensure_gids) for the engine gid_engine (nullptr: the contents are stale); the array
  // is kept when the haystack is staged again
  mutable std::mutex gid_mu;
  mutable uint32_t* d_gid = nullptr;
  mutable uint64_t gid_cap = 0;  // entries d_gid holds
  mutable const void* gid_engine = nullptr;
  // a batch's haystack (Batch::h): the batch's n_docs + 1 document byte offsets, which end the last
  // grapheme of every document (d_off is tagged and has no closing entry per document); else nullptr
  const uint64_t* d_doc_off = nullptr;
  uint64_t n_docs = 0;
  int device = 0;
  uint64_t failed_n = 0;  // graphemes counted by a failed restage (stage_haystack_device), for the error
};

// A batch of independent documents staged on the device (stage_kernels.hip stage_batch_device,
// fac.h fac_batch_*). `h` holds the concatenated bytes and, for the non-ASCII documents only, their
// graphemes in document order: h.d_off[g] = global byte | document << kDocTagShift, h.d_text32[g];
// h.ascii = every document is ASCII, h.n = graphemes of the non-ASCII documents. The descriptors of
// the non-empty documents (d_segs, d_prefix: SearchParams::segs / seg_prefix) are written by the
// device; byte_base carries the document tag, so every record's start and end come back tagged
// (local_byte subtracts the tagged byte_base from the tagged d_off, and adds it back).
constexpr uint32_t kDocTagShift = 40;
constexpr uint64_t kBatchMaxDocs = 1ull << 24;
struct BatchTri {  // per document: graphemes of a non-ASCII document, windows, 1 if not empty
  uint64_t u, w, s;
};
struct Batch {
  Haystack h;
  uint64_t n_docs = 0;
  uint64_t* d_offsets = nullptr;  // n_docs + 1 document byte offsets
  bool own_offsets = false;
  uint64_t offsets_cap = 0;       // entries an owned d_offsets holds
  // per-document scratch, kept when staged again: flags[n_docs] (bit 0 invalid UTF-8, bit 1 not
  // ASCII), tri_in / tri_ex[n_docs + 1] (counts and their exclusive scan), scal[8]
  void* d_meta = nullptr;
  size_t meta_cap = 0;
  uint32_t* d_flags = nullptr;
  BatchTri* d_tri_in = nullptr;
  BatchTri* d_tri_ex = nullptr;
  unsigned long long* d_scal = nullptr;
  SegDesc* d_segs = nullptr;
  uint64_t* d_prefix = nullptr;
  uint64_t seg_cap = 0;
  uint64_t n_segs = 0;   // non-empty documents
  uint64_t windows = 0;  // start windows of all documents
  uint64_t err_doc = 0, err_graphemes = 0;  // of a failed staging
  // the pre-filter's document-start bitmap (prefilter_kernels.hip batch_prefilter_windows): one
  // bit per byte of h.d_utf8, set at the first byte of every non-empty document; built by the first
  // pre-filtered search after a staging and kept until the batch is staged again
  mutable std::mutex dstart_mu;
  mutable uint32_t* d_dstart = nullptr;
  mutable uint64_t dstart_cap = 0;  // words d_dstart holds
  mutable bool dstart_ready = false;
  // fac_batch_allow_unicode_prefilter: a batch with non-ASCII documents may take the pre-filtered
  // calls. Its scan runs in the batch's start-window space (d_prefix: a symbol is a byte of an ASCII
  // document, a grapheme of any other); d_sstart is that space's document-start bitmap, one bit per
  // symbol, built and kept as d_dstart is (same mutex). The flag survives a restage in place.
  bool unicode_pf = false;
  // fac_batch_allow_unicode_mappings: an engine with multi-character mappings may take this batch
  // even if it holds non-ASCII documents (their grapheme ids: batch_grapheme_ids_kernel). Kept
  // across a restage like unicode_pf, and independent of it.
  bool unicode_map = false;
  // fac_batch_require_boundaries: the sides (FAC_BOUNDARY_*) of every raw record that must be
  // boundaries of its document for the record to reach the apply; 0 = off. Kept across a restage
  // like the opt-ins above. The window batches of stream.cpp never set it.
  int boundaries = 0;
  // fac_batch_require_anchors: the sides (FAC_ANCHOR_*) at which every raw record must touch its
  // document's ends to reach the apply; 0 = off. Kept across a restage like the boundary mask and
  // independent of it. The window batches of stream.cpp never set it.
  int anchors = 0;
  // stream_windows_docs: the documents are long (256 KiB windows), so stage_batch_device segments
  // the non-ASCII ones by chunks of the text (batch_seg_chunk_kernel) instead of one thread each.
  // The staged batch is the same either way.
  bool long_docs = false;
  mutable uint32_t* d_sstart = nullptr;
  mutable uint64_t sstart_cap = 0;  // words d_sstart holds
  mutable bool sstart_ready = false;
};
// stage_kernels.hip: the pre-filter's symbol id of all b.windows symbols of a batch with non-ASCII
// documents (ascii_id[byte] in an ASCII document, the GraphemeTable lookup of the folded grapheme in
// any other), written to d_ids on st (asynchronous): batch_symbol_ids_kernel
int batch_symbol_ids_device(const Engine& e, const Batch& b, uint8_t* d_ids, hipStream_t st, std::string& err);
// stage_kernels.hip: sets bit d_prefix[k] of d_bits (zeroed by the caller) for every non-empty document k
int batch_symbol_starts_device(const Batch& b, uint32_t* d_bits, hipStream_t st, std::string& err);
// stage_kernels.hip: d_out[i] = d_in[0] + ... + d_in[i - 1] for i < n, on st (asynchronous)
int exclusive_sum_u64(const uint64_t* d_in, uint64_t* d_out, uint64_t n, hipStream_t st, std::string& err);
// stage_kernels.hip: stages the documents [d_offsets[d], d_offsets[d + 1]) of b.h.d_utf8 (b.h.len
// bytes, b.n_docs, b.d_offsets set by the caller) on st; synchronous
int stage_batch_device(const Engine& e, Batch& b, hipStream_t st, std::string& err);
void free_batch(Batch& b);
// rank_kernels.hip: FuzzyMatches::apply per document on the n tagged records at d_a (d_b: scratch of
// n). Kept records, tag cleared and rebased to their document, go to *res (d_a or d_b) grouped by
// document; d_doc_off (device, n_docs + 1) receives the CSR index
int apply_batch_device(const Engine& e, fac_match* d_a, fac_match* d_b, uint64_t n, const uint64_t* d_offsets,
                       uint64_t n_docs, int order, int overlap, const uint64_t* unique_ids, hipStream_t s,
                       uint64_t* d_doc_off, fac_match** res, uint64_t* n_res, std::string& err);
// boundary_kernels.hip: the whole-token filter of a batch's n raw records at d_in (tagged, as the
// search left them): the records whose sides `sides` are boundaries of their own document go to
// d_out (room for n, not overlapping d_in) in no particular order, *n_kept of them. d_count: 8 bytes
// of device scratch. Reads b.h.d_utf8 inside the record's document only; synchronises once.
int boundary_filter_device(const Batch& b, int sides, const fac_match* d_in, uint64_t n, fac_match* d_out,
                           unsigned long long* d_count, hipStream_t s, uint64_t* n_kept, std::string& err);
// anchor_kernels.hip (fac.h "Anchored matches"). anchor_filter_device: boundary_filter_device's contract
// with the anchor rule (start == the document's first byte for FAC_ANCHOR_START, end == its end for
// FAC_ANCHOR_END); it reads b.d_offsets and never the text. lookup_table_device: row d of the
// n_docs x k table at d_table takes the first min(k, m_d) of document d's applied records (d_recs
// with the CSR index d_doc_off), the other slots the filler (pattern_index = FAC_UNMATCHED, all else
// 0); d_found[d] = min(k, m_d). Asynchronous on s.
int anchor_filter_device(const Batch& b, int sides, const fac_match* d_in, uint64_t n, fac_match* d_out,
                         unsigned long long* d_count, hipStream_t s, uint64_t* n_kept, std::string& err);
int lookup_table_device(const fac_match* d_recs, const uint64_t* d_doc_off, uint64_t n_docs, uint32_t k, fac_match* d_table,
                        uint32_t* d_found, hipStream_t s, std::string& err);
// f32 total_cmp as an unsigned key on the host (wave_util.h total_key is the device's)
inline uint32_t total_key_host(float f) {
  uint32_t b;
  std::memcpy(&b, &f, 4);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
// count_kernels.hip (fac.h "Term counts of a batch"): the group-by of a batch's applied records
// (d_recs, document-relative, grouped by document, with their CSR index d_doc) by key(pattern_index).
// Documents are handled by their record count m_d: m_d <= lane_max one lane each, m_d <= group_max
// one workgroup each, the rest through a device merge sort. The ceilings passed at run time may be
// lower than these built-in ones (fac_diag_count_terms), never higher.
constexpr uint32_t kCountLaneMax = 8;      // records a lane sorts in registers
constexpr uint32_t kCountGroupMax = 2048;  // records a workgroup sorts in LDS: 32 KiB + 16 B (count_kernels.hip)
constexpr uint32_t kCountHistKeys = 4096;  // n_keys up to which the totals use a 32 KiB LDS histogram per workgroup
void call_scratch_give(void* p, hipStream_t s);  // (declared with the pool below)
struct CountPlan {
  hipStream_t s = nullptr;
  void* mem[8] = {};  // call scratch, given back on s
  const fac_match* d_recs = nullptr;
  const uint64_t* d_doc = nullptr;
  const uint32_t* d_keys = nullptr;  // device copy of the pattern -> key table, or NULL (key = pattern)
  uint64_t n_docs = 0;
  uint32_t lane_max = 0, group_max = 0;
  // documents per tier (the group tier in two lists: up to 64 records, and more), records of the sorted tier
  uint64_t n_lane = 0, n_wave = 0, n_group = 0, n_sorted = 0, sorted_recs = 0;
  uint32_t *d_lane = nullptr, *d_wave = nullptr, *d_group = nullptr, *d_sorted = nullptr;  // the document lists
  uint64_t* d_term_off = nullptr;  // n_docs + 1: the CSR index into the terms
  void* d_entries = nullptr;       // sorted tier: the sorted entries, their run ids, run heads, per-document base
  uint64_t *d_hid = nullptr, *d_hpos = nullptr, *d_aux = nullptr;
  uint64_t total = 0;  // terms of the whole batch
  ~CountPlan() {
    for (void* p : mem)
      if (p) call_scratch_give(p, s);
  }
};
// Pass 1: classifies the documents, counts every document's distinct keys, scans the counts into
// plan.d_term_off and reads plan.total back (synchronises twice). keys: host array of n_patterns
// entries or NULL; uploaded here. FAC_E_UNSUPPORTED: a document with 2^32 or more records.
int count_plan_device(const fac_match* d_recs, const uint64_t* d_doc, uint64_t n_docs, const uint32_t* keys,
                      uint64_t n_patterns, uint32_t lane_max, uint32_t group_max, hipStream_t s, CountPlan& plan,
                      std::string& err);
// Pass 2: writes the plan.total terms to d_terms, one 16-byte store each (asynchronous on plan.s).
int count_write_device(const CountPlan& plan, fac_term* d_terms, std::string& err);
// The corpus totals of n_terms terms: zeroes d_totals[0, n_keys) and adds every term (asynchronous on s).
int count_totals_device(const fac_term* d_terms, uint64_t n_terms, uint64_t n_keys, fac_term_total* d_totals, hipStream_t s,
                        std::string& err);
// The rule on the host (fac.h fac_count_records): terms in ascending key order.
void count_records_host(const fac_match* recs, uint64_t n, const uint32_t* keys, std::vector<fac_term>& out);
// The whole-token mask of a stream task (fac.h fac_stream_open_opts) and the stream's text before
// the task's first byte: the last before_len (<= kBoundaryCarry) bytes of it, on the host;
// more_before: the stream has text before those.
struct StreamBoundary {
  int sides = 0;
  const uint8_t* before = nullptr;
  uint32_t before_len = 0;
  bool more_before = false;
};
// boundary_kernels.hip: the same filter for the raw records of a stream task, tagged with their
// window (bits kWinTagShift and up). Window w is bytes [d_src[w], d_src[w] + d_len[w]) of the task's
// text_len bytes at d_text. d_doc_off NULL: the records hold offsets of that text (the ASCII union
// path); else offsets of the expanded text, where window w's copy begins at d_doc_off[w] (the
// window-documents path). Neighbours are read from d_text -- never from the expanded copies, which
// have no left context -- and, left of its byte 0, from the before_len bytes at d_before, whose
// front is the start of the stream or far enough away (StreamBoundary). The end side is decided
// inside the window: a record that ends at its window's end is kept.
struct StreamFilter {
  int sides = 0;
  const uint8_t* d_text = nullptr;
  uint64_t text_len = 0;
  const uint64_t* d_src = nullptr;
  const uint64_t* d_len = nullptr;
  const uint64_t* d_doc_off = nullptr;
  uint64_t n_windows = 0;
  const uint8_t* d_before = nullptr;
  uint32_t before_len = 0;
};
int stream_boundary_filter_device(int device, const StreamFilter& f, const fac_match* d_in, uint64_t n, fac_match* d_out,
                                  unsigned long long* d_count, hipStream_t s, uint64_t* n_kept, std::string& err);

// replace_kernels.hip: the splice of a batch (fac.h fac_replace_batch; matches.rs:165-188 per
// document). A replacement table holds per pattern {offset into d_bytes, byte length}, the length
// kReplaceKeep for "keep the matched text" (the callback's None, matches.rs:180-183).
constexpr uint32_t kReplaceKeep = 0xFFFFFFFFu;
constexpr uint32_t kReplaceTile = 4096;  // output bytes one workgroup of replace_copy_kernel owns
// A template entry (fac_replacements_create_templates) also has an insert position k in d_ins: its
// piece is bytes [0, k) of the entry, the matched text, bytes [k, len). kReplaceNoInsert: a plain
// entry. d_ins exists only for tables that hold a template; the others run the kernels without it.
constexpr uint32_t kReplaceNoInsert = 0xFFFFFFFFu;
struct ReplaceTable {
  int device = 0;
  uint64_t n_patterns = 0;
  uint2* d_tab = nullptr;
  uint8_t* d_bytes = nullptr;
  uint32_t* d_ins = nullptr;
};
// The plan of one call: per kept record {output offset of its piece within its document's output
// (bit 63: the guard skipped the record), source offset its preceding gap starts at}, and the
// n_docs + 1 output offsets. Scratch comes from the stream's pool and goes back with the plan.
void call_scratch_give(void* p, hipStream_t s);  // (declared with the pool below)
struct ReplacePlan {
  hipStream_t s = nullptr;
  void* mem = nullptr;
  ulonglong2* d_plan = nullptr;
  uint64_t* d_out_off = nullptr;
  uint64_t total = 0;       // output bytes of the whole batch
  uint64_t n_replaced = 0;  // records the splice applied
  ~ReplacePlan() {
    if (mem) call_scratch_give(mem, s);
  }
};
// d_recs / d_doc_off: apply_batch_device's result (kept records in (document, start, acceptance)
// order, document-relative, and their CSR index). Plans the splice and scans the output lengths on
// s; synchronises once to read total and n_replaced back.
int replace_plan_device(const Batch& b, const ReplaceTable& t, const fac_match* d_recs, uint64_t n_recs,
                        const uint64_t* d_doc_off, hipStream_t s, ReplacePlan& plan, std::string& err);
// Writes the plan.total output bytes to d_out (asynchronous on plan.s).
int replace_copy_device(const Batch& b, const ReplaceTable& t, const fac_match* d_recs, const uint64_t* d_doc_off,
                        const ReplacePlan& plan, uint8_t* d_out, std::string& err);

// The plan of a run of consecutive stream windows (fac.h fac_replace_windows_staged_device, the
// replace stream's tasks; stream.rs:465-517 + ReplaceCursor::emit_window, :645-705): the run's source
// range [e_in, e_out) of the resident text is one document of replace_copy_kernel. d_recs holds the
// records rebased to e_in, d_view that document's {byte range, record range, output range} (d_out_off
// points at the last pair).
struct StreamReplacePlan : ReplacePlan {
  fac_match* d_recs = nullptr;
  uint64_t* d_view = nullptr;
  uint64_t e_out = 0;      // ReplaceCursor::emitted after the run's last window
  uint64_t n_skipped = 0;  // records the guard `match_start < emitted` skipped (:671)
};
// recs: the owned records of the windows in window order (sorted here by (start, end) within a window
// where the ranking left them otherwise, stream.rs:515), win_off their CSR index (n_windows + 1),
// commit each window's commit point, e_in the cursor on entry; every offset is a byte of the resident
// text. Uploads them, runs the carry chain over the windows and the per-record plan on s;
// synchronises once to read total, e_out and the counts back.
int replace_stream_plan_device(const ReplaceTable& t, std::vector<fac_match>& recs, const std::vector<uint64_t>& win_off,
                               const std::vector<uint64_t>& commit, uint64_t e_in, hipStream_t s, StreamReplacePlan& plan,
                               std::string& err);
// Writes the plan.total output bytes, spliced from d_text, to d_out (asynchronous on plan.s).
int replace_stream_copy_device(const uint8_t* d_text, const ReplaceTable& t, const StreamReplacePlan& plan, uint8_t* d_out,
                               std::string& err);

#if defined(__HIPCC__)
// The 16 output bytes a lane of an output-stationary byte mover owns (replace_copy_kernel,
// piece_copy_kernel), little-endian in two registers, filled run by run.
struct Chunk16 {
  uint64_t lo = 0, hi = 0;
  uint32_t filled = 0;
};
// One byte, or `take` bytes of a run (they fit: filled + take <= 16).
__device__ inline void chunk_put(Chunk16& c, uint64_t v) {
  if (c.filled < 8) c.lo |= v << (8 * c.filled);
  else c.hi |= v << (8 * (c.filled - 8));
  ++c.filled;
}
__device__ inline void chunk_put(Chunk16& c, const uint8_t* __restrict__ src, uint32_t take) {
  for (uint32_t t = 0; t < take; ++t) chunk_put(c, src[t]);
}
// The whole chunk from one run (filled == 0, 16 bytes readable at src): aligned words and byte
// shifts (a misaligned source is the rule; the fifth word is read only when it holds one of the 16
// bytes).
__device__ inline void chunk_load16(Chunk16& c, const uint8_t* __restrict__ src) {
  const uint32_t a = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 3u);
  const uint32_t* w = reinterpret_cast<const uint32_t*>(src - a);
  const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = a ? w[4] : 0u;
  const uint32_t o0 = __builtin_amdgcn_alignbyte(w1, w0, a), o1 = __builtin_amdgcn_alignbyte(w2, w1, a);
  const uint32_t o2 = __builtin_amdgcn_alignbyte(w3, w2, a), o3 = __builtin_amdgcn_alignbyte(w4, w3, a);
  c.lo = (uint64_t)o0 | ((uint64_t)o1 << 32);
  c.hi = (uint64_t)o2 | ((uint64_t)o3 << 32);
  c.filled = 16;
}
// One 16-byte store for a full chunk when `out` is 16-byte aligned (wide), byte stores otherwise.
__device__ inline void chunk_store(const Chunk16& c, uint8_t* __restrict__ out, int wide) {
  if (wide && c.filled == 16) {
    *reinterpret_cast<uint4*>(out) =
        make_uint4((uint32_t)c.lo, (uint32_t)(c.lo >> 32), (uint32_t)c.hi, (uint32_t)(c.hi >> 32));
  } else {
    for (uint32_t t = 0; t < c.filled; ++t) out[t] = (uint8_t)(t < 8 ? c.lo >> (8 * t) : c.hi >> (8 * (t - 8)));
  }
}
// One output piece of a table entry t (ins: its insert position) for a match whose text is `tlen`
// bytes is up to three source runs: pre = rep[t.x, t.x + k), text = the match's bytes,
// suf = rep[t.x + k, t.x + len). A plain entry is pre alone (k = len), "keep" is text alone, and
// any run may be empty (replace_copy_kernel<true>, extract_copy_kernel).
__device__ inline uint64_t piece_len(uint2 t, uint32_t ins, uint64_t tlen) {
  if (t.y == kReplaceKeep) return tlen;
  return (uint64_t)t.y + (ins != kReplaceNoInsert ? tlen : 0);
}
// Run `run` (0 pre, 1 text, 2 suf) of that piece: where its bytes start and how many they are.
__device__ inline void piece_run(uint2 t, uint32_t ins, const uint8_t* __restrict__ rep,
                                 const uint8_t* __restrict__ text, uint64_t tlen, int run,
                                 const uint8_t*& src, uint64_t& rl) {
  const bool keep = t.y == kReplaceKeep, slot = keep || ins != kReplaceNoInsert;
  const uint32_t len = keep ? 0u : t.y, k = keep ? 0u : (ins != kReplaceNoInsert ? ins : len);
  if (run == 0) {
    src = rep + t.x;
    rl = k;
  } else if (run == 1) {
    src = text;
    rl = slot ? tlen : 0;
  } else {
    src = rep + t.x + k;
    rl = len - k;
  }
}
#endif

// extract_kernels.hip: the strings of a batch's kept records (fac.h fac_extract_batch;
// FuzzyMatches::matched_strings, matches.rs:513-515, or the table's piece per record). Item i is
// the string of record i: bytes [d_item_off[i], d_item_off[i + 1]) of the output.
struct ExtractPlan {
  hipStream_t s = nullptr;
  void* mem = nullptr;
  uint64_t* d_item_off = nullptr;  // n_items + 1 output offsets
  uint64_t* d_src = nullptr;       // per item: the global byte its matched text starts at
  uint64_t n_items = 0;
  uint64_t total = 0;  // output bytes of the whole batch
  ~ExtractPlan() {
    if (mem) call_scratch_give(mem, s);
  }
};
// d_recs / d_doc_off: apply_batch_device's result, any order and overlap. t NULL: every item is its
// record's matched text. Writes and scans the item lengths on s; synchronises once to read total.
int extract_plan_device(const Batch& b, const ReplaceTable* t, const fac_match* d_recs, uint64_t n_recs,
                        const uint64_t* d_doc_off, hipStream_t s, ExtractPlan& plan, std::string& err);
// Writes the plan.total output bytes to d_out (asynchronous on plan.s).
int extract_copy_device(const Batch& b, const ReplaceTable* t, const fac_match* d_recs, const ExtractPlan& plan,
                        uint8_t* d_out, std::string& err);

// segment_kernels.hip: the segmentation helpers of a batch (fac.h fac_segment_batch and
// fac_render_batch; matches.rs:218-594 per document). The modes are fac.h's FAC_RENDER_*, and
// kSegmentRecords for the segments themselves.
constexpr int kRenderStripPrefix = 0, kRenderStripSuffix = 1, kRenderSegmentText = 2, kSegmentRecords = 3;
constexpr uint32_t kSegmentTile = 4096;  // output bytes one workgroup of piece_copy_kernel owns
// The plan of one call: the n_docs + 1 segment offsets (segment_text and the segments), the
// n_docs + 1 output byte offsets (the render modes) and, for a strip, the global byte each
// document's kept part starts at. Scratch comes from the stream's pool and goes back with the plan.
struct SegmentPlan {
  hipStream_t s = nullptr;
  int mode = 0;
  void* mem = nullptr;
  void* mem_pieces = nullptr;  // segment_text: one piece per segment (render_copy_device)
  uint64_t* d_seg_off = nullptr;
  uint64_t* d_out_off = nullptr;
  uint64_t* d_src = nullptr;
  uint64_t n_segs = 0;  // segments of the whole batch
  uint64_t total = 0;   // output bytes of the whole batch
  ~SegmentPlan() {
    if (mem_pieces) call_scratch_give(mem_pieces, s);
    if (mem) call_scratch_give(mem, s);
  }
};
// d_recs / d_doc_off: apply_batch_device's result, as for replace_plan_device. Walks every
// document's records and scans the counts and lengths the mode needs on s; synchronises once to
// read n_segs and total back.
int segment_plan_device(const Batch& b, int mode, const fac_match* d_recs, const uint64_t* d_doc_off, hipStream_t s,
                        SegmentPlan& plan, std::string& err);
// Writes the plan.n_segs segments to d_out, 8-byte aligned (asynchronous on plan.s).
int segment_write_device(const Batch& b, const fac_match* d_recs, const uint64_t* d_doc_off, const SegmentPlan& plan,
                         fac_match* d_out, std::string& err);
// Writes the plan.total output bytes of a render mode to d_out (asynchronous on plan.s).
int render_copy_device(const Batch& b, const fac_match* d_recs, const uint64_t* d_doc_off, SegmentPlan& plan,
                       uint8_t* d_out, std::string& err);

// Where a search delivers its records: a host vector (internal callers), a pooled pinned host
// buffer handed to the C ABI caller (fac_search_staged / fac_search_raw: no page faults on the
// D2H, result_alloc below), or the caller's device buffer (fac_search_staged_device: records stay
// in HBM for the RCCL gather). `n` counts every record; with a device buffer only the first
// dev_cap are written.
struct MatchSink {
  std::vector<fac_match>* vec = nullptr;
  fac_match* pinned = nullptr;
  uint64_t pinned_cap = 0;
  fac_match* dev = nullptr;
  uint64_t dev_cap = 0;
  uint64_t n = 0;
};
// result buffers (api.cpp): large ones come from a pool of pinned host buffers that
// fac_matches_free returns to the pool; small ones are malloc'd. result_free takes either.
fac_match* result_alloc(uint64_t n_records);
void result_free(void* p);
int sink_append_device(MatchSink& s, const fac_match* d_src, uint64_t cnt, hipStream_t stream, std::string& err);
int sink_append_host(MatchSink& s, const fac_match* src, uint64_t cnt, hipStream_t stream, std::string& err);

// builder.cpp
int build_engine(const fac_pattern* pats, uint64_t n, const fac_config* cfg, Engine& e, std::string& err);
// a node's children (folded graphemes, insertion order) -> their transitions-map iteration order
std::vector<uint32_t> transitions_order(const std::vector<std::u32string>& children);
// search_kernels.hip
int launch_search(const Engine& e, const Haystack& h, const std::vector<SegDesc>& segs, float thr,
                  hipStream_t stream, std::vector<fac_match>& out, fac_stats* stats, std::string& err);
// ab_prefix: the running auto-beam total (queue.len() summed) of the windows before this call's
// first window, for a shard of one haystack (search.rs:1096-1103); 0 for a whole search
int launch_search_sink(const Engine& e, const Haystack& h, const std::vector<SegDesc>& segs, float thr,
                       hipStream_t stream, uint64_t ab_prefix, MatchSink& sink, fac_stats* stats, std::string& err);
// The batch entry's search: the segment and window-prefix arrays are already on the device
// (Batch::d_segs / d_prefix: non-empty segments, w_end <= n) and only the totals are known to the
// host, so a million-document batch costs no per-document host loop and no descriptor upload.
// Auto-beam engines read the descriptors back and take launch_search_sink's per-segment loop.
// The prefix cache is gated by the batch's own rule, not by windows per segment.
int launch_search_batch(const Engine& e, const Batch& b, float thr, hipStream_t stream, MatchSink& sink,
                        fac_stats* stats, std::string& err);
// Prefiltered::raw of every document of a batch, all ASCII or opted in (Batch::unicode_pf;
// prefilter.rs:304-374 per document; ks:
// prefilter_ks' edit budgets): one bitap pass over the concatenated bytes with the automaton reset
// and the coverage cut at every document start (batch_prefilter_windows), then each merged window
// searched as a haystack of its own, one segment of one launch_pass (launch_search_batch_windows).
// The descriptors and their window prefix are written by the device, ascending by start (so by
// document); the host reads back the two totals. The records come out tagged with their document
// like launch_search_batch's. Scratch comes from the stream's pool and goes back with the struct.
struct BatchWindows {
  hipStream_t s = nullptr;
  SegDesc* d_segs = nullptr;    // n descriptors: ascii, text_base = global byte, byte_base tagged
  uint64_t* d_prefix = nullptr;  // n + 1 entries
  uint64_t n = 0;        // merged windows of all documents
  uint64_t windows = 0;  // their lengths summed: the start windows to search
  // records the search is expected to return, where the caller knows better than the launcher's
  // windows / 64 (anchored windows: one window per document, a record or more each); 0 = no hint.
  // A first buffer too small costs a second search, never a record.
  uint64_t out_hint = 0;
  // want_tri (a batch with non-ASCII documents, fac_batch_prefilter_windows): d_tri receives per
  // window {document, start, end} in document-relative symbols (bytes of an ASCII document,
  // graphemes of any other), which the descriptor of a slice no longer tells
  bool want_tri = false;
  uint64_t* d_tri = nullptr;
  ~BatchWindows() {
    if (d_segs) call_scratch_give(d_segs, s);
    if (d_prefix) call_scratch_give(d_prefix, s);
    if (d_tri) call_scratch_give(d_tri, s);
  }
};
int batch_prefilter_windows(const Engine& e, const Batch& b, const std::vector<uint32_t>& ks, hipStream_t stream,
                            BatchWindows& out, fac_stats* stats, std::string& err);
int launch_search_batch_windows(const Engine& e, const Batch& b, const BatchWindows& w, float thr, hipStream_t stream,
                                MatchSink& sink, fac_stats* stats, std::string& err);
// anchor_kernels.hip: the batch's own descriptors (Batch::d_segs, untouched) copied with the window
// range narrowed to the start windows an anchored record can come from: [0, 1) when `sides` holds
// FAC_ANCHOR_START, the last min(n, max_match_graphemes + 2) for FAC_ANCHOR_END alone. n, hay_len,
// avail, text_base and the tagged byte_base stay the document's. One segment per non-empty document,
// never empty; synchronises once (the window total).
int anchor_windows_device(const Engine& e, const Batch& b, int sides, hipStream_t st, BatchWindows& out, std::string& err);
// auto-beam pass 1 alone: sum of queue.len() over the windows of `segs` searched unbeamed
int auto_beam_total(const Engine& e, const Haystack& h, const std::vector<SegDesc>& segs, float thr,
                    hipStream_t stream, uint64_t& total, std::string& err);
// diagnostics knobs: FAC_* environment variables are honoured only with FAC_DIAGNOSTICS=1 set, so
// a stray variable in a user's environment never changes the search path
const char* diag_env(const char* name);
// the host copies of a staged haystack (Haystack::utf8, ::starts), fetched once from the device
int ensure_host(const Haystack& h, std::string& err);
// the grapheme ids of a Unicode haystack (or of a batch's non-ASCII documents) for an engine with
// mappings: h.d_gid, written by the device on st on first use and complete on return
int ensure_gids(const Engine& e, const Haystack& h, hipStream_t st, std::string& err);
// stage_kernels.hip: Engine::gid_of's id (0 = not in the dictionary) of every grapheme of h, looked
// up in e.gid_tab and written to d_ids[0, h.n) on st (asynchronous): grapheme_ids_kernel, or
// batch_grapheme_ids_kernel for a batch's haystack
int grapheme_ids_device(const Engine& e, const Haystack& h, uint32_t* d_ids, hipStream_t st, std::string& err);
// largest grapheme count a haystack may have (u32::MAX, search.rs:198-201; lowered only by the
// diagnostics knob FAC_GRAPHEME_LIMIT so tests can reach SearchError::HaystackTooLarge)
uint64_t grapheme_limit();
// A set of lazily grown device scratch buffers for the search launcher. The engine owns one (leased
// by whichever call gets it first); a streaming search owns one per in-flight window, bound to the
// worker thread that searches it (scratch_bind) so concurrent windows never hipMalloc per call.
struct ScratchSet {
  static constexpr int kSlots = 64;
  std::mutex mu;
  void* p[kSlots] = {};
  size_t n[kSlots] = {};
  hipStream_t aux = nullptr;  // this set's low-priority second stream (prefix-cache level-1 build)
};
void scratch_bind(ScratchSet* s);  // this thread's searches use `s` (nullptr: the engine's)
void scratch_free(ScratchSet& s);
int aux_priority();  // the stream priority of a set's (and the engine's) aux stream
// Short-lived call scratch (rank kernels, stream-window record buffers), one process-wide pool: a
// block given back on stream s is handed out again only for work on s (same device), whose order
// makes the reuse safe without the device-wide synchronisation a hipFree implies (a per-call
// hipMalloc/hipFree stalled every other stream once per stream window). At most 2 GiB / 64 blocks
// are kept (oldest freed first); fac_trim_scratch / fac_engine_free release them.
void* call_scratch_take(size_t bytes, hipStream_t s, hipError_t* e);
void call_scratch_give(void* p, hipStream_t s);
void call_scratch_trim();                         // frees every kept block
void call_scratch_release_stream(hipStream_t s);  // before the library destroys stream s

// stream.cpp: the WindowReader state (stream.rs:77-159), the windows in flight and the matches
// ready to hand out. Windows are cut on the host and searched by `depth` worker threads, each with
// its own HIP stream and scratch: window k + 1's upload, segmentation and search overlap window k's
// (double buffering); results are handed out in window order.
struct StreamTask;
struct StreamWorker;
struct StreamCore {
  const Engine* e = nullptr;
  float threshold = 0.f;
  uint64_t window = 256 * 1024;  // DEFAULT_WINDOW (stream.rs:61)
  uint64_t overlap = 1;
  std::vector<uint8_t> buf;
  uint64_t base = 0, total = 0;
  uint64_t carry = 0;  // bytes the last window left in the buffer (its text after the commit point)
  uint64_t valid_end = 0;  // stream offset up to which the bytes are known valid UTF-8 (a character boundary)
  bool done = false;
  StreamTask* pending = nullptr;  // windows cut but not yet dispatched (one batch)
  std::vector<fac_match> ready;
  std::vector<uint8_t> ready_text;  // matched bytes of `ready`, concatenated
  static constexpr uint32_t depth = 2;
  StreamWorker* workers[depth] = {};
  std::vector<StreamTask*> inflight;  // window order
  uint64_t seq = 0;
  uint64_t handed = 0;  // commit point of the last window whose matches were handed out
  int failed = 0;
  std::string fail_msg;
  uint64_t batch_bytes = 32ull << 20;  // text a task collects before it is dispatched (FAC_STREAM_BATCH_BYTES)
  uint64_t read = 64 * 1024;  // the reader's read() size (stream.rs:102-158; FAC_STREAM_READ_BYTES)
  // every window's text is searched as Prefiltered::search (fac_stream_open_ex; prefilter.rs:304-374)
  bool prefilter = false;
  // whole-token matches (fac.h fac_stream_open_opts): the FAC_BOUNDARY_* mask every window's raw
  // records are filtered by before they are ranked, 0 = off; `tail`: the stream's last
  // kBoundaryCarry bytes before buf[0], kept only with a mask (a task's left context)
  int boundaries = 0;
  std::vector<uint8_t> tail;
  // start windows of the segments handed to the search launcher, for the windows handed out so far
  uint64_t windows_searched = 0;
  // tasks handed out so far that were searched in one pass (stream_windows_batch or
  // stream_windows_docs) and window by window (fac_stream_task_counts)
  uint64_t tasks_batched = 0, tasks_single = 0;
  // a task with non-ASCII text is searched as one batch of window documents (FAC_STREAM_WINDOW_DOCS=0,
  // a diagnostics knob, turns that off: such a task's windows are then searched one by one)
  bool window_docs = true;
  // replace mode (fac_replace_stream_*): the table, the output ready to hand out, the totals of the
  // tasks handed out, and ReplaceCursor::emitted (stream.rs:645-648) as it passes from task to task:
  // cur_emitted is the cursor after task cur_seq - 1, and task cur_seq plans next
  const ReplaceTable* table = nullptr;
  std::vector<uint8_t> ready_out;
  uint64_t written = 0, applied = 0, skipped = 0;
  std::mutex cur_mu;
  std::condition_variable cur_cv;
  uint64_t cur_seq = 0, cur_emitted = 0;
  bool cur_failed = false;
};

// table: NULL for a search stream; else the stream replaces (the table outlives the stream)
StreamCore* stream_open(const Engine& e, float threshold, uint64_t window, const ReplaceTable* table = nullptr,
                        bool prefilter = false, int boundaries = 0);
int stream_feed(StreamCore& s, const uint8_t* data, uint64_t len, bool eof, std::string& err);
void stream_close(StreamCore* s);
uint64_t stream_committed(const StreamCore& s);  // commit point of the windows handed out so far
// staging of the bytes at h.d_utf8 on the device (stage_kernels.hip): mode -2 checks the UTF-8 and
// decides is_ascii, 0 stages Unicode graphemes, 1 ASCII (asynchronous after its count sync)
int stage_device(const Engine& e, Haystack& h, hipStream_t st, std::string& err, int mode);
// graphemes of a staged haystack that start before byte b (a grapheme boundary), synchronously on st
int graphemes_before(const Haystack& h, uint64_t b, hipStream_t st, uint64_t& out, std::string& err);
// stage_kernels.hip: the lookup table of `keys` (folded grapheme, id), built on the device
int grapheme_table_build(const std::vector<std::pair<std::u32string, uint32_t>>& keys, GraphemeTable& t, hipStream_t st,
                         std::string& err);
void grapheme_table_free(GraphemeTable& t);
// The pre-filter's symbol id (prefilter.rs:262-280; 0 = other) of graphemes [g0, g1) of a staged
// Unicode haystack, written to d_ids[0, g1 - g0) on st (asynchronous): symbol_ids_kernel
int symbol_ids_device(const Engine& e, const Haystack& h, uint64_t g0, uint64_t g1, uint8_t* d_ids, hipStream_t st,
                      std::string& err);
// prefilter_kernels.hip: the same for ASCII text (prefilter.rs:253-258): d_ids[i] = ascii_id[d_utf8[i]], i < n
int transcode_ascii_device(const Engine& e, const uint8_t* d_utf8, uint64_t n, uint8_t* d_ids, hipStream_t st,
                           std::string& err);
// The descriptors of graphemes [gs, ge) x n of a staged Unicode haystack, each searched as a text of
// its own (search_raw on a slice re-decides is_ascii, search.rs:196, prefilter.rs:349-350):
// slice_desc_kernel on st, then the n descriptors are read back (synchronous)
int slice_descs_device(const Haystack& h, const std::vector<std::pair<uint64_t, uint64_t>>& spans, hipStream_t st,
                       std::vector<SegDesc>& out, std::string& err);
int apply_matches(const Engine& e, std::vector<fac_match>& v, int order, int overlap, const uint64_t* unique_ids,
                  std::string& err);
// stream.rs window_matches' tail on the device (rank_kernels.hip): the n raw records of one window
// at d_a (d_b: scratch of n) ranked sorted().non_overlapping(), those starting before `commit` bytes
// into the window (which starts at byte byte_base of the staged text) rebased to stream offset `base`
// and written to d_out; *n_owned their count (FAC_E_OUTPUT_CAPACITY if it exceeds cap)
int window_owned_device(const Engine& e, fac_match* d_a, fac_match* d_b, uint64_t n, uint64_t byte_base, uint64_t commit,
                        uint64_t base, hipStream_t s, fac_match* d_out, uint64_t cap, uint64_t* n_owned, std::string& err);
// A stream window of a batch: its text starts at staged byte byte_base, it owns the matches starting
// before commit bytes into it, and byte_base maps to stream offset base. A batch's ASCII segments
// carry their window in the bits of SegDesc::byte_base from kWinTagShift up, so every record's start
// and end come back tagged (the kernels only add byte offsets to byte_base for ASCII text).
struct WinOwn {
  uint64_t byte_base, commit, base;
};
constexpr uint32_t kWinTagShift = 40;
// win_off (optional): the CSR index of the windows into `out`, wins.size() + 1 entries
void windows_owned_host(const Engine& e, std::vector<fac_match>& recs, const std::vector<WinOwn>& wins,
                        std::vector<fac_match>& out, std::vector<uint64_t>* win_off = nullptr);
// api.cpp: a batch of stream windows (g_begin, g_end, commit_bytes, base) x n of a whole staged ASCII
// haystack searched in one pass; FAC_E_UNSUPPORTED when the batch does not qualify (see there)
// win_off (optional): the CSR index of the windows into `owned`, n_windows + 1 entries
int stream_windows_batch(const Engine& e, const Haystack& h, const uint64_t* wins, uint64_t n_windows, float threshold,
                         bool prefilter, hipStream_t st, std::vector<fac_match>& owned, fac_stats* stats, std::string& err,
                         std::vector<uint64_t>* win_off = nullptr, uint64_t* searched = nullptr,
                         const StreamBoundary* sb = nullptr);  // sb with sides != 0: whole-token matches of a stream
// stage_kernels.hip: the expanded text of a stream task. Window w is bytes [d_src[w], d_src[w] +
// d_len[w]) of the text_len bytes at d_text (every range inside the text, checked by the caller;
// d_len has a closing entry); the n_windows + 1 document offsets go to d_offsets (exclusive sums of
// d_len) and the windows' bytes, one after the other, to the `total` bytes at d_out (asynchronous)
int stream_gather_device(const uint8_t* d_text, uint64_t text_len, const uint64_t* d_src, const uint64_t* d_len,
                         uint64_t n_windows, uint64_t total, uint8_t* d_out, uint64_t* d_offsets, hipStream_t st,
                         std::string& err);
// rank_kernels.hip: the commit cut of a batch of window documents. d_recs / d_doc_off:
// apply_batch_device's result for NonOverlapping (a document's records in start order, document-
// relative). Window w owns the records that start before d_commit[w], a prefix of its group; they go
// to `owned` in window order with d_add[w] added to start and end, win_off receives their CSR index
// (n_windows + 1). Only those records and the index are copied to the host (synchronous).
int windows_owned_device(const fac_match* d_recs, uint64_t n_recs, const uint64_t* d_doc_off, uint64_t n_windows,
                         const uint64_t* d_commit, const uint64_t* d_add, hipStream_t s, std::vector<fac_match>& owned,
                         std::vector<uint64_t>& win_off, std::string& err);
// api.cpp: a task of stream windows searched as one batch whose document w is window w's text
// (wins as for stream_windows_batch, byte offsets into the text_len bytes at d_text): the expanded
// text is gathered into wd.b (owned by the caller, restaged in place), staged per document, searched
// through the batch front (pre-filter, one launch, per-document rank and overlap walk) and cut at
// the commit points on the device. A window that fails staging gives its search_raw error.
struct WindowDocs {
  Batch b;                // h.d_utf8 (the expanded text) and d_offsets are the batch's own
  uint64_t text_cap = 0;  // bytes h.d_utf8 holds
};
// FAC_E_UNSUPPORTED (nothing done): more than 2^24 windows or 2^40 expanded bytes.
int stream_windows_docs(const Engine& e, WindowDocs& wd, const uint8_t* d_text, uint64_t text_len, const uint64_t* wins,
                        uint64_t n_windows, float threshold, bool prefilter, hipStream_t st, std::vector<fac_match>& owned,
                        std::string& err, std::vector<uint64_t>& win_off, uint64_t* searched,
                        const StreamBoundary* sb = nullptr);
// prefilter_kernels.hip: merged bitap windows (prefilter.rs:319-342) of a text view of a staged haystack (view.ascii:
// bytes [text_base, text_base + n) of h.d_utf8; else graphemes [text_base, text_base + n)); windows
// in the view's local grapheme coordinates
// diagnostics: beam_select(_lds) alone on key arrays (tests; fac_diag_beam_select)
int diag_beam_select(const float* keys, const uint64_t* offs, uint64_t count, uint32_t bw, int32_t lds,
                     int32_t sel_limit, uint32_t* perm, std::string& err);
int prefilter_windows(const Engine& e, const Haystack& h, const SegDesc& view, const std::vector<uint32_t>& ks,
                      hipStream_t stream, std::vector<std::pair<uint64_t, uint64_t>>& windows, fac_stats* stats,
                      std::string& err);
// the same for a batch of stream windows of the view (wins: [lo, hi) text positions, sorted, each
// overlapping only its neighbours): one scan of the view, every window's merged bitap windows as if
// its text were searched alone; run_win = each merged window's stream window. FAC_E_UNSUPPORTED
// when the tables need the packed full scan.
int prefilter_windows_ex(const Engine& e, const Haystack& h, const SegDesc& view, const std::vector<uint32_t>& ks,
                         hipStream_t stream, const std::vector<std::pair<uint64_t, uint64_t>>* wins,
                         std::vector<std::pair<uint64_t, uint64_t>>& windows, std::vector<uint32_t>* run_win,
                         fac_stats* stats, std::string& err);
// api.cpp: Prefiltered::raw on a text view of a staged haystack (prefilter.rs:304-374); the plain
// search of the view where the reference falls back. searched (optional): += the start windows of
// the segments handed to the search launcher
int prefiltered_view(const Engine& e, const Haystack& h, const SegDesc& view, float threshold, hipStream_t stream,
                     std::vector<fac_match>& merged, fac_stats* stats, std::string& err, uint64_t* searched = nullptr);
// device_state.cpp. force_ascii: -1 decide from the bytes (search.rs:196), 0 Unicode graphemes, 1 ASCII bytes (a
// shard of a haystack whose global is_ascii is already known)
int stage_haystack(const Engine& e, const uint8_t* utf8, uint64_t len, Haystack& h, std::string& err,
                   int force_ascii = -1, hipStream_t stream = nullptr);
// search_raw's staging of bytes already in device memory (borrowed, not copied): the UTF-8 check,
// is_ascii, segmentation and folding on the device; h may hold buffers of an earlier staging.
// mode -2: decide is_ascii from the bytes; 1 / 0: ASCII / Unicode graphemes as given (a shard of a
// haystack whose global is_ascii is known; Unicode bytes are UTF-8 checked)
int stage_haystack_device(const Engine& e, const uint8_t* d_utf8, uint64_t len, Haystack& h, std::string& err,
                          hipStream_t stream, int mode = -2);
// start byte of the n-th grapheme counted from the end of s[0, len) (UAX #29, the whole text's
// segmentation; stream.rs:134-139 grapheme_indices(true).rev().nth(n - 1)); false if it has fewer
bool nth_grapheme_from_end(const uint8_t* s, uint64_t len, uint64_t n, uint64_t& off);
// shard planning (unicode.cpp): p is a grapheme boundary whose segmentation does not depend on
// anything before it (previous char ASCII and not CR, char at p neither Extend, ZWJ nor SpacingMark;
// or the char at p starts a cluster in every context: GCB Other, not ExtPict, no InCB class, and
// the previous char is not Prepend)
bool safe_cut(const uint8_t* s, uint64_t n, uint64_t p);
// str::is_ascii (search.rs:196), eight bytes at a time
bool ascii_only(const uint8_t* s, uint64_t n);
void free_haystack(Haystack& h);
int upload_engine(Engine& e, std::string& err);
void free_engine_device(Engine& e);

}  // namespace fac
