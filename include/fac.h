/* fac.h — C ABI of the MI355X-native fuzzy Aho–Corasick engine (libfac.so).
 *
 * Drop-in boundary for the hot path of kakserpom/fuzzy-aho-corasick-rs v0.5.0 (reference at
 * /root/reference). Everything public in the crate funnels through one crate-private seam,
 *
 *     pub(crate) fn search_raw(&'a self, haystack: &'a str, similarity_threshold: f32)
 *         -> Result<FuzzyMatches<'a>, SearchError>                       (src/search.rs:187-191)
 *
 * plus the engine constructor `FuzzyAhoCorasickBuilder::build` (src/builder.rs:181) and the
 * pre-filter wrapper `Prefiltered::search` (src/prefilter.rs:135-155). The entry points below are
 * exactly what a Rust `extern "C"` block (or any FFI) would bind to replace those; see
 * INTEGRATION.md for the binding a maintainer would add. Plain pointers and sizes only; no C++ or
 * torch types cross this boundary. All functions are reentrant; an engine is immutable after
 * fac_build and may be shared across host threads (structs.rs:528-567).
 *
 * Return codes (SearchError is #[non_exhaustive], src/error.rs:7-17, so new codes follow the
 * reference's own convention):
 *   FAC_OK                      0
 *   FAC_E_HAYSTACK_TOO_LARGE    1   SearchError::HaystackTooLarge{graphemes} (search.rs:198-201)
 *   FAC_E_INVALID             100   bad argument (NULL, invalid UTF-8, beam_width == 0, ...)
 *   FAC_E_UNSUPPORTED         101   configuration outside the GPU path (> 64 mapping transitions
 *                                   at one node, > 2^26 nodes, a beam or a node fan-out past the
 *                                   largest frontier ring of 2^20 states, ...) — never a silent CPU
 *                                   fallback
 *   FAC_E_HIP                 102   HIP runtime error (fac_last_error() has the text)
 *   FAC_E_NO_DEVICE           103   no usable MI355X (gfx950) device
 *   FAC_E_OOM                 104   host or device allocation failure
 *   FAC_E_CAPACITY            105   a per-window device work buffer overflowed even after the
 *                                   automatic retries: one window's frontier past the largest
 *                                   HBM rung (2^20 states), or past what the HBM frontier budget
 *                                   holds; fac_last_error() names the bound. The budget: at most
 *                                   1 GiB of device scratch, allocated when a search first needs
 *                                   an HBM rung; like the engine's other scratch it stays bound
 *                                   to the engine (or stream worker) until that is freed
 *   FAC_E_OUTPUT_CAPACITY     106   the caller's device output buffer is too small; *n_out holds
 *                                   the record count needed (fac_search_staged_ex)
 *   FAC_E_INTERNAL            107   unexpected internal error (fac_last_error() has the text)
 *
 * Diagnostics: the library reads FAC_* environment knobs (kernel variants, prefix-cache levels,
 * FAC_GRAPHEME_LIMIT, ...) only when FAC_DIAGNOSTICS=1 is set; otherwise the search path depends
 * on the arguments alone. FAC_OUT_CAP0, FAC_ECAP0 and FAC_SPILL_CAP0 (each >= 1) set the first size
 * of a search pass's record buffer, per-window best lists and spill list, whose overflow re-runs
 * the pass with a larger buffer: results never depend on them. FAC_STREAM_BATCH_BYTES (>= 1) replaces
 * the 32 MiB of text a stream (fac_stream_*, fac_replace_stream_*) collects into one device task:
 * results never depend on it either.
 */
#ifndef FAC_H
#define FAC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FAC_OK 0
#define FAC_E_HAYSTACK_TOO_LARGE 1
#define FAC_E_INVALID 100
#define FAC_E_UNSUPPORTED 101
#define FAC_E_HIP 102
#define FAC_E_NO_DEVICE 103
#define FAC_E_OOM 104
#define FAC_E_CAPACITY 105
#define FAC_E_OUTPUT_CAPACITY 106
#define FAC_E_INTERNAL 107

#define FAC_LIMIT_NONE (-1)

/* FuzzyLimits (src/structs.rs:293-299), already finalized (structs.rs:319-335):
 * each field is a count 0..255 or FAC_LIMIT_NONE. */
typedef struct fac_limits {
  int32_t insertions;
  int32_t deletions;
  int32_t substitutions;
  int32_t swaps;
  int32_t edits;
} fac_limits;

/* One Pattern (src/structs.rs:598-610). `custom_unique_id` only matters for host-side
 * overlap resolution and is not passed. */
typedef struct fac_pattern {
  const char* utf8; /* pattern text, valid UTF-8 */
  uint64_t len;     /* bytes */
  float weight;     /* Pattern::weight, default 1.0 */
  int32_t has_limits;
  fac_limits limits; /* per-pattern limits, finalized; used iff has_limits */
} fac_pattern;

/* One multi-character mapping rule (a, b, score), builder.rs:30-31, 116-132: either side may
 * stand in for the other at penalty substitution * (1 - score), counted as one substitution. */
typedef struct fac_mapping {
  const char* a; /* UTF-8 */
  uint64_t a_len;
  const char* b; /* UTF-8 */
  uint64_t b_len;
  float score;
} fac_mapping;

/* Builder state (src/builder.rs:22-33, FuzzyPenalties structs.rs:370-393). */
typedef struct fac_config {
  int32_t case_insensitive;
  int32_t has_limits;   /* FuzzyAhoCorasickBuilder::fuzzy(...) called */
  fac_limits limits;    /* finalized global limits */
  float penalty_insertion;
  float penalty_deletion;
  float penalty_substitution;
  float penalty_swap;
  uint64_t beam_width;  /* 0 = None (exact exploration) */
  int32_t has_auto_beam;
  uint64_t auto_beam_budget;
  uint64_t auto_beam_width;
  float min_symbol_similarity;
  /* Custom Similarity (structs.rs:30-54); NULL = the crate's DEFAULT_SIMILARITY
   * (builder.rs:492-526). similarity_ascii is a 128x128 row-major table indexed [a][b];
   * the pair list holds entries with a or b >= 128. */
  const float* similarity_ascii;
  uint64_t n_similarity_pairs;
  const uint32_t* similarity_pairs; /* 2*n code points (a, b) */
  const float* similarity_pair_values;
  /* Multi-character mappings (builder.rs:108-132, mapping / mapping_scored): applied
   * bidirectionally; precomputed per trie node like builder.rs:383-442. */
  uint64_t n_mappings;
  const struct fac_mapping* mappings;
  int32_t device; /* HIP device ordinal for this engine's tables */
} fac_config;

/* Owned match record: the crate's OwnedMatch/StreamMatch POD (src/stream.rs:719-745), 32 bytes,
 * identical on host, device and the RCCL wire. `start`/`end` are byte offsets into the haystack;
 * the host rebuilds `text = haystack[start..end]`. */
typedef struct fac_match {
  uint64_t start;
  uint64_t end;
  uint32_t pattern_index;
  float similarity;
  uint8_t insertions;
  uint8_t deletions;
  uint8_t substitutions;
  uint8_t swaps;
  uint8_t edits;
  uint8_t pad[3];
} fac_match;

/* Per-call device statistics (filled when the pointer is non-NULL). */
typedef struct fac_stats {
  double kernel_ms;        /* HIP-event time of the window search kernel(s) on the call's stream */
  double prefilter_ms;     /* HIP-event time of the bitap scan + window merge (0 if unused) */
  uint64_t kernel_launches;
  uint64_t windows;        /* start windows searched */
  uint64_t states_popped;  /* BFS states popped by the search kernel (work diagnostic) */
  uint64_t graphemes;      /* haystack graphemes */
  uint64_t bytes;          /* haystack UTF-8 bytes */
  uint64_t retries;        /* capacity retries */
  double cache_ms;         /* HIP-event time of the prefix cache: key counts, snapshot builds, per-window lookups */
  uint64_t states_cached;  /* pops replayed from prefix-cache snapshots (not in states_popped) */
  double lane_ms;          /* HIP-event time of the lane-serial search of small resumed windows */
  uint64_t lane_windows;   /* windows finished by the lane-serial kernel */
} fac_stats;

typedef struct fac_engine fac_engine;
typedef struct fac_haystack fac_haystack;
typedef struct fac_replacements fac_replacements; /* a replacement table: "Batched replace" below */

/* Last error text of the calling thread ("" if none). */
const char* fac_last_error(void);

/* FuzzyAhoCorasickBuilder::build (builder.rs:181-484): builds the trie, fail-link output merge
 * and prune coefficients on the host and uploads the device tables to cfg->device. */
int fac_build(const fac_pattern* patterns, uint64_t n_patterns, const fac_config* cfg,
              fac_engine** out);
void fac_engine_free(fac_engine* engine);
/* Frees the prefix-cache snapshots the engine keeps from search to search (the snapshot pool, up to
 * FAC_RC_POOL_MB, and its key directories); the next search builds every key again. Waits for a search
 * that is using them. fac_engine_free frees them too. */
void fac_engine_drop_prefix_cache(fac_engine* engine);
/* Frees the device blocks the library keeps for reuse between calls (per-call scratch of the
 * pre-filter, ranking and stream windows; at most 2 GiB are kept, fac_engine_free trims too). */
void fac_trim_scratch(void);

/* FuzzyAhoCorasick::search_raw (search.rs:187-395): best-per-(start,end,pattern) matches at or
 * above `threshold`, unordered. *out is allocated by the library (fac_matches_free). On
 * FAC_E_HAYSTACK_TOO_LARGE, *err_graphemes receives the grapheme count. */
int fac_search_raw(const fac_engine* engine, const uint8_t* utf8, uint64_t len, float threshold,
                   fac_match** out, uint64_t* n_out, uint64_t* err_graphemes);
void fac_matches_free(fac_match* matches);

/* FuzzyAhoCorasick::with_prefilter + Prefiltered (prefilter.rs:113-155). */
int fac_prefilter_active(const fac_engine* engine);
int fac_search_prefiltered(const fac_engine* engine, const uint8_t* utf8, uint64_t len,
                           float threshold, fac_match** out, uint64_t* n_out,
                           uint64_t* err_graphemes);

/* FuzzyAhoCorasick::max_match_graphemes (stream.rs:213-253). */
uint64_t fac_max_match_graphemes(const fac_engine* engine);

/* Device-resident haystacks (bench / sharded multi-GPU). fac_haystack_stage performs the
 * search_raw staging (is_ascii, grapheme segmentation + folding, search.rs:196-203/296-302)
 * and uploads the result to the engine's device; the staged haystack can then be searched
 * repeatedly with no host->device traffic. */
int fac_haystack_stage(const fac_engine* engine, const uint8_t* utf8, uint64_t len,
                       fac_haystack** out, uint64_t* err_graphemes);
/* search_raw's staging of UTF-8 bytes that are already in device memory (`d_utf8`, a device
 * pointer on the engine's device; borrowed, not copied: keep it alive and unchanged while the
 * haystack is used): the UTF-8 check (the C ABI's stand-in for `&str`), is_ascii, UAX #29
 * segmentation and folding, all on the device (search.rs:196-203, 296-302), ordered on `stream`
 * (a hipStream_t; NULL = the engine's) and complete on return. `*hay`: NULL to create a haystack,
 * or one returned earlier by this function for the same engine, whose device buffers are then
 * reused (staging again per search costs no allocation). Errors as fac_haystack_stage; on error
 * `*hay` is left as passed. */
int fac_haystack_stage_device(const fac_engine* engine, const uint8_t* d_utf8, uint64_t len, void* stream,
                              fac_haystack** hay, uint64_t* err_graphemes);
uint64_t fac_haystack_graphemes(const fac_haystack* hay);
/* Byte start of every staged grapheme (the device segmentation's result, for tests / hosts that
 * map windows to bytes). Writes up to `cap` entries, returns the grapheme count. */
uint64_t fac_haystack_grapheme_starts(const fac_haystack* hay, uint64_t* out, uint64_t cap);
/* Tests and hosts: the folded first code point of every staged grapheme (search.rs:406-412: its
 * lowercase's first code point for a case-insensitive engine, else the code point itself), as the
 * device staging wrote it. Writes up to `cap` entries, returns the grapheme count. An ASCII haystack
 * has no such array (its bytes are searched as they are): nothing is written and 0 is returned. */
uint64_t fac_haystack_text_chars(const fac_haystack* hay, uint32_t* out, uint64_t cap);
/* Tests and hosts: the bitap pre-filter's symbol id of every staged grapheme (prefilter.rs:247-281;
 * ids 1..255 in first-seen order over the patterns' folded graphemes, 0 = no pattern grapheme),
 * computed on the device: the table lookup of the folded code-point sequence for a Unicode
 * haystack, the per-byte table for an ASCII one. Writes up to `cap` ids to the host buffer `out`;
 * returns the grapheme count, -1 if the engine has no filter (fac_prefilter_active == 0), or minus
 * the error code. `stream` is a hipStream_t (NULL = the engine's stream). */
int64_t fac_haystack_symbol_ids(const fac_engine* engine, const fac_haystack* hay, void* stream, uint8_t* out,
                                uint64_t cap);
/* Tests and hosts, engines with multi-character mappings: the id of one grapheme (its UTF-8 bytes)
 * in the engine's dictionary of folded graphemes -- the patterns' and the mappings' haystack sides,
 * 1-based in first-seen order; 0 = not in the dictionary, or the engine has no mappings. Computed on
 * the host (the fold of grapheme.rs:61-63 and a hash-map lookup): the reference the device ids below
 * are tested against. */
uint32_t fac_engine_grapheme_id(const fac_engine* engine, const uint8_t* utf8, uint64_t len);
/* Tests and hosts: that id for every grapheme of a staged Unicode haystack, as the search of an
 * engine with mappings reads it: looked up on the device by the first search (or this call) after a
 * staging and kept with the haystack for that engine. Writes up to `cap` ids to the host buffer `out`;
 * returns the grapheme count, -1 if the engine has no mappings, or minus the error code. An ASCII
 * haystack has no such array (its bytes index a 128-entry table): nothing is written and 0 is
 * returned. `stream` is a hipStream_t (NULL = the engine's stream). */
int64_t fac_haystack_grapheme_ids(const fac_engine* engine, const fac_haystack* hay, void* stream, uint32_t* out,
                                  uint64_t cap);
void fac_haystack_free(fac_haystack* hay);

/* Search start windows [window_begin, window_end) of a staged haystack (window_end is clamped
 * to the grapheme count). Searching every window reproduces search_raw; disjoint window ranges
 * give disjoint match sets (the best-map key holds the start byte), which is how the host shards
 * one haystack across GPUs. `stream` is a hipStream_t (NULL = the engine's stream). */
int fac_search_staged(const fac_engine* engine, const fac_haystack* hay, uint64_t window_begin,
                      uint64_t window_end, float threshold, void* stream, fac_match** out,
                      uint64_t* n_out, fac_stats* stats);

/* Extended staged search. Records go to the host (*out, fac_matches_free) or, with device_out set,
 * straight into that device buffer of device_cap records on the engine's device (no host copy: the
 * multi-GPU gather sends them over RCCL from there); *n_out is the record count either way, and
 * FAC_E_OUTPUT_CAPACITY means the buffer was too small (grow it to *n_out and search again).
 * auto_beam_prefix: for a shard of one haystack, the running auto-beam total (sum of queue.len())
 * of every window before this shard (search.rs:1096-1103; fac_auto_beam_total), 0 otherwise. */
typedef struct fac_search_args {
  uint64_t window_begin;
  uint64_t window_end;
  float threshold;
  void* stream;
  uint64_t auto_beam_prefix;
  void* device_out;
  uint64_t device_cap;
} fac_search_args;
int fac_search_staged_ex(const fac_engine* engine, const fac_haystack* hay, const fac_search_args* args,
                         fac_match** out, uint64_t* n_out, fac_stats* stats);

/* Auto-beam pass 1 alone (search.rs:1096-1103): the sum of queue.len() over the start windows
 * [window_begin, window_end) searched unbeamed. A sharded search of an auto-beam engine exchanges
 * these totals so every shard switches the beam on at the same global window as search_raw. */
int fac_auto_beam_total(const fac_engine* engine, const fac_haystack* hay, uint64_t window_begin, uint64_t window_end,
                        float threshold, void* stream, uint64_t* total);

/* Sharding one haystack over n_shards GPUs. fac_shard_plan cuts the bytes into
 * contiguous shards at grapheme boundaries whose segmentation needs no left context (any byte of
 * an ASCII haystack; otherwise after an ASCII non-CR character, before a character that is not
 * Extend/ZWJ/SpacingMark; host-only, no device needed) and returns plan = {a, b, e, flags}: the shard owns the start windows of
 * bytes [a, b) and must stage bytes [a, e), e = b plus max_match_graphemes() + 2 graphemes (the
 * stream overlap of stream.rs:256-258 and the text[j+1] lookahead; max_match_graphemes is
 * fac_max_match_graphemes(engine)), flags bit 0 = global is_ascii,
 * bit 1 = the text continues past e. is_ascii: the haystack's is_ascii if known, -1 to compute it.
 * fac_haystack_stage_shard stages such a slice: searched with fac_search_staged[_ex] it yields
 * exactly the records search_raw of the whole haystack yields for the owned start windows, at
 * global byte offsets (slice offset + base). */
int fac_shard_plan(uint64_t max_match_graphemes, const uint8_t* utf8, uint64_t len, int32_t is_ascii, uint64_t n_shards,
                   uint64_t shard, uint64_t plan[4]);
int fac_haystack_stage_shard(const fac_engine* engine, const uint8_t* utf8, uint64_t len, uint64_t owned_bytes,
                             int32_t global_ascii, int32_t open_end, uint64_t base, fac_haystack** out,
                             uint64_t* err_graphemes);
/* fac_haystack_stage_shard for a shard whose bytes [a, e) are already in device memory (`d_utf8`,
 * borrowed like fac_haystack_stage_device's, which it otherwise follows: staging on the device,
 * ordered on `stream`, complete on return; `*hay` NULL or a haystack this function staged before,
 * restaged in place). The grapheme mode is the global is_ascii; a Unicode shard's bytes are UTF-8
 * checked on the device. Replaces nothing in the reference: it is the per-step staging of the
 * sharded search_raw (search.rs:196-203, 296-302 on each rank's slice). */
int fac_haystack_stage_shard_device(const fac_engine* engine, const uint8_t* d_utf8, uint64_t len, uint64_t owned_bytes,
                                    int32_t global_ascii, int32_t open_end, uint64_t base, void* stream, fac_haystack** hay,
                                    uint64_t* err_graphemes);
/* start windows a staged haystack owns (all of them unless it is a shard) */
uint64_t fac_haystack_owned_windows(const fac_haystack* hay);
/* Strong-scaling split by key instead of by position: searches of `hay` cover only the start windows
 * whose first two (folded) characters hash to `part` of `parts` (parts = 1: all). Every window of a
 * prefix lands in one part, so each GPU's prefix cache holds whole keys -- a position
 * shard of 1/N shares its keys with every other shard and rebuilds them. The union of the parts'
 * records is the whole haystack's search_raw (windows are independent). FAC_E_UNSUPPORTED for
 * auto_beam engines (a running count over windows in order, search.rs:1096-1103). */
int fac_haystack_set_key_partition(const fac_engine* engine, fac_haystack* hay, uint32_t parts, uint32_t part);

/* One streaming window on the device (stream.rs:262-297 window_matches): the graphemes
 * [g_begin, g_end) of a staged haystack are searched as the window's text (Prefiltered::search if
 * `prefilter`, else search), ranked sorted().non_overlapping() (matches.rs), and the matches the
 * window owns (start byte < commit_bytes, relative to the window) are returned at absolute offsets
 * base + window offset. */
int fac_stream_window_staged(const fac_engine* engine, const fac_haystack* hay, uint64_t g_begin, uint64_t g_end,
                             uint64_t commit_bytes, uint64_t base, float threshold, int32_t prefilter, void* stream,
                             fac_match** out, uint64_t* n_out, fac_stats* stats);

/* fac_stream_window_staged with the owned records left in HBM (no host round trip): the window's
 * raw records are ranked sorted().non_overlapping() on the device and the owned ones (start before
 * the commit point) written, rebased to the stream offset `base`, to device_out (room for device_cap
 * records). *n_out = the owned count; FAC_E_OUTPUT_CAPACITY when it exceeds device_cap (nothing is
 * written then; grow the buffer and call again). For the multi-GPU gather of C5 (stream.rs:378-429). */
int fac_stream_window_staged_device(const fac_engine* engine, const fac_haystack* hay, uint64_t g_begin, uint64_t g_end,
                                    uint64_t commit_bytes, uint64_t base, float threshold, int32_t prefilter, void* stream,
                                    void* device_out, uint64_t device_cap, uint64_t* n_out, fac_stats* stats);

/* A batch of streaming windows (stream.rs:262-297 window_matches for each; the crate cuts them
 * DEFAULT_WINDOW = 256 KiB apart, stream.rs:65): windows[4 w .. 4 w + 3] = (g_begin, g_end,
 * commit_bytes, base) of window w, ascending g_begin, each overlapping only its neighbours. Every
 * window is searched as its own text exactly like fac_stream_window_staged_device; on an ASCII
 * haystack the batch is one pre-filter pass over the windows' union (each window's bitap automaton
 * starting at its first byte) and one search launch over every window's segments, then per-window
 * ranking and commit cut. The owned records of all windows go to device_out in window order;
 * *n_out = their count (FAC_E_OUTPUT_CAPACITY when it exceeds device_cap). */
int fac_stream_windows_staged_device(const fac_engine* engine, const fac_haystack* hay, const uint64_t* windows,
                                     uint64_t n_windows, float threshold, int32_t prefilter, void* stream, void* device_out,
                                     uint64_t device_cap, uint64_t* n_out, fac_stats* stats);

/* Streaming replace of a run of consecutive windows of a staged haystack, spliced on the device:
 * FuzzyReplacer::replace_stream's loop body (replacer.rs:35-44 over stream.rs:480-490) for the
 * windows given, with callback(m) = the table's entry for m.pattern_index (plain, "keep" or template).
 * `windows` holds fac_stream_windows_staged_device's 4-tuples, and the owned records come from that
 * call's code path (batched where the run qualifies, window by window otherwise), each window's
 * sorted by (start, end) (window_replace_matches, stream.rs:496-517). base - byte start of g_begin
 * must be the same for every window: it is the stream offset of the haystack's byte 0
 * (FAC_E_INVALID otherwise, and for an *emitted outside the staged text). Window w + 1's text starts
 * at window w's commit point, as the reader cuts them (stream.rs:140-158).
 * The windows are then walked with ReplaceCursor::emit_window (stream.rs:645-705): *emitted is
 * ReplaceCursor::emitted on entry (0 for the first call of a stream) and on return; a record that
 * starts before the cursor is skipped (:671), the others are replaced, the text between is copied
 * through from the staged haystack (it does not cross the host again), and each window flushes up to
 * its commit point (:696-702). The call writes stream bytes [*emitted on entry, *emitted on return),
 * spliced, to device_out (device_cap bytes on the engine's device): *out_len bytes, valid UTF-8;
 * *n_applied / *n_skipped (may be NULL) count the records replaced and the records the guard
 * skipped. Consecutive calls that carry *emitted give the output of one call over all the windows.
 * FAC_E_OUTPUT_CAPACITY: device_cap is too small; nothing was written, *out_len holds the bytes
 * needed and *emitted is unchanged. FAC_E_INVALID for a table of another pattern count or device,
 * FAC_E_UNSUPPORTED for an output of 2^40 bytes or more; other errors as
 * fac_stream_windows_staged_device. */
int fac_replace_windows_staged_device(const fac_engine* engine, const fac_haystack* hay, const uint64_t* windows,
                                      uint64_t n_windows, const fac_replacements* replacements, float threshold,
                                      int32_t prefilter, void* stream, uint64_t* emitted, void* device_out,
                                      uint64_t device_cap, uint64_t* out_len, uint64_t* n_applied, uint64_t* n_skipped,
                                      fac_stats* stats);

/* Prefiltered::raw on a staged haystack (prefilter.rs:146-155, 304-374): the bitap scan and the
 * window merge run on the device-resident text, each merged window is re-searched as its own
 * sub-haystack, results are best-per-(start, end, pattern) and sorted. Falls back to the full
 * search exactly where the reference does (no bitap filter, or some pattern needs k > 24). */
int fac_search_staged_prefiltered(const fac_engine* engine, const fac_haystack* hay, float threshold,
                                  void* stream, fac_match** out, uint64_t* n_out, fac_stats* stats);

/* FuzzyMatches::apply (matches.rs:7-149) on the device: rank `n` raw records in place by `order`
 * (0 Unsorted, 1 Default, 2 Greedy, 3 CoverageWeighted; matches.rs:23-81) and resolve overlaps by
 * `overlap` (0 Keep, 1 NonOverlapping, 2 NonOverlappingUnique; matches.rs:83-149). `unique_ids`
 * (NULL = the pattern index) maps a pattern index to its uniqueness key for overlap 2 (distinct keys
 * for custom_unique_id and automatic ids). The surviving records are compacted to the front of
 * `matches`, their count written to `n_out`. */
int fac_matches_apply(const fac_engine* engine, fac_match* matches, uint64_t n, int32_t order, int32_t overlap,
                      const uint64_t* unique_ids, uint64_t* n_out);

/* ---- Batches: many independent haystacks ("documents") searched in one device pass.
 *
 * The crate's answer to many documents is one Sync engine shared by threads that call search once
 * per document (structs.rs:528-567, query.rs:30); there is no search_many in the crate. A batch is
 * that loop as one call: every document is staged as if it were staged alone (UTF-8 validity,
 * is_ascii and UAX #29 segmentation are per document; a document start is start-of-text), searched
 * as its own `haystack` argument of search_raw, and ranked with FuzzyMatches::apply on its own
 * records. Staging, the segment descriptors, attribution, ranking and overlap resolution (the
 * per-document "pattern used once" set of NonOverlappingUnique included) run on the device.
 *
 * Limits of the implementation (FAC_E_UNSUPPORTED, never a partial result): at most 2^24
 * documents and fewer than 2^40 bytes in all (a record carries its document in bits 40..63 of
 * start / end while it is inside the library; the tag is cleared before records leave it). An
 * engine with multi-character mappings takes a batch that holds a non-ASCII document only when the
 * batch is opted in with fac_batch_allow_unicode_mappings (the grapheme ids of those documents are
 * then looked up on the device, each document's last grapheme ending at its document's end); without
 * the opt-in such a call gives FAC_E_UNSUPPORTED with nothing written. Auto-beam engines read the
 * segment descriptors back and run the per-segment auto-beam loop of fac_search_staged on the host.
 * Batched replace is provided (fac_replace_batch below), and so are the other segmentation helpers:
 * segment_iter and split (fac_segment_batch), strip_prefix, strip_suffix and segment_text
 * (fac_render_batch). Every one of these calls has a pre-filtered form for batches that are all
 * ASCII or opted in (fac_search_batch_prefiltered, fac_replace_batch_prefiltered, fac_segment_batch_prefiltered,
 * fac_render_batch_prefiltered below). The matched strings of a batch, or each match's replacement,
 * come from fac_extract_batch and fac_extract_batch_prefiltered. Multi-GPU batches are not provided.
 * Which entry a document is as a whole comes from fac_lookup_batch, and which entries each document
 * mentions and how often (per-document term counts, grouped on the device) from fac_count_batch and
 * fac_count_batch_prefiltered.
 *
 * Limits of the pre-filtered forms: where the filter runs, the batch must be all ASCII or opted in
 * with fac_batch_allow_unicode_prefilter. Without the opt-in one non-ASCII document gives
 * FAC_E_UNSUPPORTED with nothing written (callers may rely on that to route such batches elsewhere;
 * fac_stream_windows_staged_device keeps the same limit). An opted-in batch is scanned once in symbol
 * coordinates -- a symbol is a byte of an ASCII document and a folded grapheme of any other, "\r\n"
 * being one -- cut at document starts; each merged window of a non-ASCII document becomes the byte
 * slice of its graphemes and is searched as a haystack of its own, byte-wise when the slice is all
 * ASCII (prefilter.rs:346-350, search.rs:196). An all-ASCII batch takes the same path whether opted
 * in or not. A batch holds at most 2^32 - 1 merged windows. Staging errors stay fac_batch_stage's:
 * a document over the grapheme limit fails there, which is stricter than the crate, whose
 * Prefiltered::search only checks each merged window it searches. */
typedef struct fac_batch fac_batch;

/* Documents d = 0..n_docs-1 are bytes [offsets[d], offsets[d+1]) of utf8.
 * offsets[0] == 0, non-decreasing; empty documents allowed. Errors follow search_raw applied to
 * the documents in order: invalid UTF-8 gives FAC_E_INVALID with *err_doc = the first offending
 * document (a sequence split by a document boundary makes both documents invalid); a document over
 * the grapheme limit gives FAC_E_HAYSTACK_TOO_LARGE with *err_doc / *err_graphemes of the first
 * such document; bad offsets give FAC_E_INVALID (*err_doc untouched). */
int fac_batch_stage(const fac_engine* engine, const uint8_t* utf8, const uint64_t* offsets, uint64_t n_docs,
                    fac_batch** out, uint64_t* err_doc, uint64_t* err_graphemes);

/* Bytes and offsets already in device memory (borrowed, like fac_haystack_stage_device: keep both
 * alive and unchanged while the batch is used). total_len = offsets[n_docs]. *batch NULL, or an
 * earlier batch of this function to restage in place (its device buffers are reused). Ordered on
 * `stream` (NULL = the engine's), complete on return. On error *batch is left as passed; a batch
 * whose restage failed is empty (zero documents). */
int fac_batch_stage_device(const fac_engine* engine, const uint8_t* d_utf8, const uint64_t* d_offsets, uint64_t n_docs,
                           uint64_t total_len, void* stream, fac_batch** batch, uint64_t* err_doc,
                           uint64_t* err_graphemes);

void fac_batch_free(fac_batch* batch);
uint64_t fac_batch_docs(const fac_batch* batch);

/* Opt-in (on != 0) or back out (0, the default): the pre-filtered calls below take this batch even
 * if it holds non-ASCII documents (see "Limits of the pre-filtered forms" above). Sets a flag and
 * does no work; the flag survives a restage in place (fac_batch_stage_device with *batch set). Not
 * to be called concurrently with a search of the same batch. FAC_E_INVALID for NULL. */
int fac_batch_allow_unicode_prefilter(fac_batch* batch, int32_t on);

/* Opt-in (on != 0) or back out (0, the default): every batch call, plain or pre-filtered, of an
 * engine with multi-character mappings takes this batch even if it holds non-ASCII documents (see
 * "Limits of the implementation" above). Independent of fac_batch_allow_unicode_prefilter (an engine
 * with mappings has no filter: its pre-filtered calls are the plain ones). Sets a flag and does no
 * work; the flag survives a restage in place. Not to be called concurrently with a search of the
 * same batch. FAC_E_INVALID for NULL. */
int fac_batch_allow_unicode_mappings(fac_batch* batch, int32_t on);

/* ---- Whole-token matches. The search restarts at every grapheme, so "art" is found inside "party";
 * the crate's answer is to filter search_raw's records by their surrounding characters before
 * FuzzyMatches::apply. For a batch that filter runs on the device, between the search and the
 * per-document apply, so an in-word match never takes part in the overlap walk.
 *
 * The rule. A record (start, end) of a document doc[0, n) has two sides; `sides` is a mask of
 * FAC_BOUNDARY_START and FAC_BOUNDARY_END, and a record is kept when every requested side is a boundary.
 *  - End side: a boundary when end == n, or when the code point that begins at byte `end` is not
 *    alphanumeric. (No walk: `end` is a grapheme start.)
 *  - Start side: walk left from `start` over code points. A transparent code point -- General_Category
 *    M* (Mn, Mc, Me) and not alphanumeric: combining accents, variation selectors -- is skipped; the
 *    first other code point decides, a boundary when it is not alphanumeric. Reaching byte 0 of the
 *    document is a boundary. Having skipped 32 transparent code points without a decision is a
 *    boundary too: a stated bound on the work per record, just above the 30 non-starters of the
 *    Stream-Safe Text Format. (The walk keeps the accent of decomposed "cafe + U+0301 + bar" from passing
 *    for a word break.)
 *  - Alphanumeric is Rust's char::is_alphanumeric: the Alphabetic property, or General_Category
 *    Nd / Nl / No. '_' and '-' are boundaries, U+00B2 and U+2160 are not; U+093E (an alphabetic Mc)
 *    is alphanumeric, not transparent.
 *  - A document's start and end are boundaries whatever its neighbours in the batch hold. Empty
 *    spans follow the same rule. The rule reads the document's UTF-8 bytes only: it is the same for
 *    ASCII and non-ASCII documents and does not depend on the engine, case folding or mappings.
 *
 * fac_batch_require_boundaries sets the mask of a batch (0 = off, the default; 0..3, anything else
 * or NULL gives FAC_E_INVALID). It sets a flag and does no work; the flag survives a restage in
 * place; not to be called concurrently with a search of the same batch. Every batch call on that
 * batch, plain or pre-filtered (fac_search_batch, fac_replace_batch, fac_extract_batch,
 * fac_segment_batch, fac_render_batch and their _prefiltered forms), then returns for every document
 * apply(order, overlap) of the document's raw records with the rule applied first. With the mask
 * off the calls launch and allocate nothing for it.
 *
 * Streams are covered: fac_stream_open_opts / fac_replace_stream_open_opts take the same mask in
 * fac_stream_options::boundaries. The rule is applied per window, to the window's raw records,
 * before that window's sorted().non_overlapping() and before the ownership cut (start < commit),
 * as the batch calls apply it per document. What a window counts as "the document":
 *  - Start side: the walk to the left runs over the stream's text, not the window's. It goes on
 *    past the window's first byte into the bytes the stream read before it (a window begins at its
 *    predecessor's commit point, a grapheme boundary in the middle of the text). Only byte 0 of the
 *    stream is a boundary by position. The walk reads at most 32 code points, so the last 4 x 32 =
 *    128 bytes before a window always decide it, and that is all a device task carries over from
 *    its predecessor.
 *  - End side: decided inside the window's text. end == the window text's length is a boundary
 *    (the final window's end is the stream's end); otherwise the code point at `end` decides. A
 *    window's result is therefore a function of the window and the text before it alone, whatever
 *    the grouping of windows into device tasks or the feeding. A record that ends at a non-final
 *    window's end is never owned by that window: an owned record starts before the commit point
 *    and spans at most max_match_graphemes graphemes, and the overlap is one more than that, so at
 *    least two graphemes of the window follow it. Such a record only takes part in that window's
 *    overlap walk; the next window owns it and judges it with its real right-hand neighbour.
 *  - With the mask 0 a stream launches, allocates, uploads and carries nothing for the feature.
 * Not covered: fac_search_staged*, fac_matches_apply (which have no text) and the staged-window
 * calls of the multi-GPU C5 path, fac_stream_window[s]_staged[_device] and
 * fac_replace_windows_staged_device. */
#define FAC_BOUNDARY_START 1
#define FAC_BOUNDARY_END 2
#define FAC_BOUNDARY_WHOLE 3
int fac_batch_require_boundaries(fac_batch* batch, int32_t sides);
/* Tests and hosts: bit 0 = alphanumeric, bit 1 = transparent (never both); 0 for surrogates and
 * values above U+10FFFF. */
int32_t fac_boundary_class(uint32_t cp);
/* Tests and hosts: the rule above on the host, over one document's bytes: 1 = kept, 0 = dropped.
 * A negative value is an error: -FAC_E_INVALID for NULL text with len > 0, sides outside 0..3,
 * start > end, end > len, or an offset inside a code point (on a continuation byte). The text is
 * taken as valid UTF-8 and not checked beyond that; no byte outside [0, len) is read. */
int32_t fac_boundary_ok(const uint8_t* utf8, uint64_t len, uint64_t start, uint64_t end, int32_t sides);
/* Tests and hosts: the stream rule above on the host. utf8[0, len) is a window's text and
 * before[0, before_len) the stream's text that precedes it; more_before != 0 says the stream has
 * text before `before`, so reaching its front is not the stream's start. Returns and errors as
 * fac_boundary_ok (before == NULL with before_len > 0 included); also -FAC_E_INVALID when the
 * start side's walk reaches the front of `before` undecided while more_before != 0, which cannot
 * happen with before_len >= 128. `before` may begin inside a code point: its leading continuation
 * bytes are never read as a code point. */
int32_t fac_boundary_ok_after(const uint8_t* before, uint64_t before_len, int32_t more_before, const uint8_t* utf8,
                              uint64_t len, uint64_t start, uint64_t end, int32_t sides);

/* ---- Anchored matches. The batch calls answer "where in this document does a dictionary entry
 * occur?"; for a column of names or titles the question is as often "which entry IS this string?"
 * (a fuzzy join, normalising a column against canonical names). The crate's route is
 * FuzzyMatches::retain between search_raw and apply (matches.rs:417); for a batch that filter runs
 * on the device at the same point as the whole-token filter above, and it lets the search skip the
 * start windows that cannot contribute.
 *
 * The rule. `sides` is a mask of FAC_ANCHOR_START and FAC_ANCHOR_END. A raw record (start, end) of a
 * document doc[0, n) is kept when start == 0, if START is requested, and end == n, if END is
 * requested. Offsets are bytes within the record's own document, ASCII or not. Empty spans follow
 * the same rule; an empty document has no windows and so no records. The rule reads only the record
 * and the document's two offsets: never the text, and it does not depend on the engine. It runs on
 * the complete raw record set before apply(order, overlap), together with the whole-token filter
 * when both masks are set (both are pure predicates, so their order does not matter): for every
 * document the result of a batch call is apply(order, overlap) of {r in search_raw(doc) : rule(r)},
 * and of {r in Prefiltered::raw(doc) : rule(r)} for a pre-filtered call.
 *
 * The window restriction. Start windows of one search_raw are independent (fac_search_staged:
 * disjoint window ranges give disjoint record sets). A record with start == 0 can only come from
 * start window 0, and a record that ends at the document's end only from the last
 * fac_max_match_graphemes() windows. A plain (not pre-filtered) call on an engine that is not
 * auto-beam-only therefore searches one window per non-empty document for START and WHOLE, and for
 * END alone the last min(n, T) windows, T = fac_max_match_graphemes() + 2 (the bound and margin of
 * fac_shard_plan's halo); fac_stats.windows reports the windows searched. The records are the
 * unrestricted call's: the restriction only leaves out windows whose records the rule drops.
 * Auto-beam-only engines (has_auto_beam, beam_width == 0) search every window -- the crate's
 * running total runs over all windows in order (search.rs:1096-1103), so leaving windows out would
 * move the switch point -- and pre-filtered calls keep their merged windows; both get the filter.
 *
 * fac_batch_require_anchors sets the mask of a batch (0 = off, the default; 0..3, anything else or
 * NULL gives FAC_E_INVALID). It sets a flag and does no work; the flag survives a restage in place;
 * not to be called concurrently with a search of the same batch. It is independent of the boundary
 * mask and of both Unicode opt-ins, and honoured by fac_search_batch, fac_replace_batch,
 * fac_extract_batch, fac_segment_batch, fac_render_batch and their _prefiltered forms. With the mask
 * 0 the calls launch, allocate and upload nothing for it. Streams and fac_search_staged* are not
 * covered (a window has no document end). */
#define FAC_ANCHOR_START 1
#define FAC_ANCHOR_END 2
#define FAC_ANCHOR_WHOLE 3
int fac_batch_require_anchors(fac_batch* batch, int32_t sides);
/* Tests and hosts: the rule above for a record (start, end) of a document of doc_len bytes: 1 =
 * kept, 0 = dropped; -FAC_E_INVALID for sides outside 0..3, start > end or end > doc_len. */
int32_t fac_anchor_ok(uint64_t doc_len, uint64_t start, uint64_t end, int32_t sides);

/* Tests and hosts: as fac_haystack_grapheme_ids for the graphemes of the batch's non-ASCII documents,
 * in document order (fac_batch_doc_graphemes of those documents, concatenated). An all-ASCII batch
 * writes nothing and returns 0. Needs no opt-in. */
int64_t fac_batch_grapheme_ids(const fac_engine* engine, const fac_batch* batch, void* stream, uint32_t* out, uint64_t cap);

/* Tests and hosts: document d's grapheme count, is_ascii, and document-relative grapheme byte
 * starts (writes up to `cap` entries, returns the count). */
uint64_t fac_batch_doc_graphemes(const fac_batch* batch, uint64_t d, int32_t* is_ascii);
uint64_t fac_batch_grapheme_starts(const fac_batch* batch, uint64_t d, uint64_t* out, uint64_t cap);
/* Tests and hosts: the folded first code point of every grapheme of document d (as
 * fac_haystack_text_chars; 0 and nothing written for an ASCII document). */
uint64_t fac_batch_text_chars(const fac_batch* batch, uint64_t d, uint32_t* out, uint64_t cap);

typedef struct fac_batch_args {
  float threshold;
  int32_t order;               /* as fac_matches_apply */
  int32_t overlap;             /* as fac_matches_apply */
  const uint64_t* unique_ids;  /* as fac_matches_apply (host array, one key per pattern) */
  void* stream;
  void* device_out;            /* optional: records stay in HBM */
  uint64_t device_cap;
  uint64_t* device_doc_offsets; /* optional: n_docs+1 entries on the device */
} fac_batch_args;

/* Records grouped by document, ascending document index. start/end are relative to the record's
 * own document. doc_offsets (caller's host array, n_docs+1 entries) is the CSR index into the
 * records. Within a document: the order FuzzyMatches::apply(order, overlap) gives. For
 * Unsorted+Keep the order within a document is unspecified; Unsorted with an overlap mode walks a
 * document's records in (start, end, pattern_index) order (the crate walks its hash map's order).
 * Records go to the host (*out, fac_matches_free) or, with device_out set, into that device buffer
 * of device_cap records; FAC_E_OUTPUT_CAPACITY: the buffer is too small, *n_out holds the count
 * needed and nothing was written. */
int fac_search_batch(const fac_engine* engine, const fac_batch* batch, const fac_batch_args* args, fac_match** out,
                     uint64_t* n_out, uint64_t* doc_offsets, fac_stats* stats);

/* fac_search_batch with the crate's bit-parallel pre-filter per document: for every document d the
 * result is engine.with_prefilter().search(doc_d, opts) (prefilter.rs:113-155, 304-374) -- the
 * document transcoded alone, bitap_windows for every pattern from the initial state at its first
 * symbol, the windows sorted and merged (adjacent ones merge), search_raw on each merged window as a
 * haystack of its own, then FuzzyMatches::apply per document. No automaton state, coverage or merged
 * window crosses a document boundary. One pass over the batch's bytes finds every document's
 * windows; the descriptors of the merged windows are written by the device and searched in one
 * launch. The result is not always fac_search_batch's: a merged window is its own search_raw call,
 * so an auto-beam engine's running total restarts per merged window (one segment each, searched by
 * the per-segment loop fac_search_batch uses for such engines).
 * Where the reference falls back to the full search -- no filter (fac_prefilter_active == 0, which
 * covers engines with mappings), or k_for above 24 for some pattern at this threshold -- the call is
 * fac_search_batch exactly, for any batch. Otherwise arguments, contract, errors and limits are
 * fac_search_batch's plus the "all ASCII, or opted in" limit above. stats: prefilter_ms = device time of the scan,
 * verify and runs; windows = the start windows searched, the merged windows' lengths summed. */
int fac_search_batch_prefiltered(const fac_engine* engine, const fac_batch* batch, const fac_batch_args* args,
                                 fac_match** out, uint64_t* n_out, uint64_t* doc_offsets, fac_stats* stats);

/* Tests and diagnostics: the merged windows fac_search_batch_prefiltered searches, as
 * (document, start, end) triples with document-relative symbol offsets -- bytes for an ASCII
 * document, graphemes for any other (an opted-in batch), the coordinates of Prefiltered's merged
 * windows, ends clamped to the document -- ascending by document, then by start. Writes up to `cap` triples to `out` and returns their count, -1 where the reference falls
 * back to the full search, or minus the error code (every FAC_E_* that can occur here is >= 100). */
int64_t fac_batch_prefilter_windows(const fac_engine* engine, const fac_batch* batch, float threshold, void* stream,
                                    uint64_t* out, uint64_t cap);

/* ---- Dictionary lookup of a batch ("Anchored matches" above): the dense form a join wants. Row d
 * of an n_docs x k table holds the first min(k, m_d) records of apply(order, Keep) over document d's
 * FAC_ANCHOR_WHOLE-anchored raw records (m_d of them), start and end relative to the document; the
 * remaining slots hold pattern_index = FAC_UNMATCHED, similarity 0, all counts 0 and start = end = 0.
 * found (host array of n_docs entries, may be NULL) receives min(k, m_d). The three orders are total
 * orders (matches.rs:24-81) and with WHOLE a document has at most one record per pattern, so the
 * table is fully determined. order 0 is taken as 1 (Default), as the replace calls take it.
 * The table goes to the host (*out, fac_matches_free; n_docs * k records) or, with device_out set,
 * into that device buffer of device_cap records (out may then be NULL); FAC_E_OUTPUT_CAPACITY: the
 * buffer holds fewer than n_docs * k records, and nothing was written. FAC_E_INVALID: k == 0, a NULL
 * argument, a bad order; FAC_E_UNSUPPORTED: n_docs * k >= 2^40. The call applies WHOLE whatever the
 * batch's own anchor mask says and does not modify the batch; the batch's boundary mask and Unicode
 * opt-ins apply as in fac_search_batch, and so do its other errors and limits. There is no
 * _prefiltered form: one window per document leaves the pre-filter nothing to save. */
typedef struct fac_lookup_args {
  float threshold;
  int32_t order;  /* as fac_matches_apply; 0 = 1 */
  uint32_t k;     /* slots per document, > 0 */
  void* stream;
  void* device_out; /* optional: the table stays in HBM */
  uint64_t device_cap;
} fac_lookup_args;
int fac_lookup_batch(const fac_engine* engine, const fac_batch* batch, const fac_lookup_args* args, fac_match** out,
                     uint32_t* found, fac_stats* stats);

/* ---- Term counts of a batch: "which entries does each document mention, and how often" -- the
 * document-term matrix of a column against the dictionary, grouped on the device.
 *
 * For every document d, ms = engine.search(doc_d, opts) exactly as fac_search_batch computes it: the
 * options are taken as passed (no `segmented` normalisation, as in fac_extract_batch), the batch's
 * boundary mask, anchor mask and both Unicode opt-ins are honoured, and errors and limits are
 * fac_search_batch's. A pattern -> key table folds surface forms into entities: with keys == NULL,
 * key(p) = p and n_keys must be 0 or the engine's pattern count; otherwise keys is a host array of
 * one uint32_t per pattern, each < n_keys, and n_keys <= 2^32 - 1. A key >= n_keys gives
 * FAC_E_INVALID before anything runs. keys is uploaded per call.
 * Document d's terms are the groups of ms by key(pattern_index), in ascending key order. A document
 * without kept records owns an empty range. The term set does not depend on the order of ms, so
 * Unsorted + Keep is fully determined here; the order only matters through the overlap walk. A
 * document with 2^32 or more kept records gives FAC_E_UNSUPPORTED; a partial result is never returned. */
typedef struct fac_term {
  uint32_t key;
  uint32_t count;          /* records of the group */
  float    best_similarity;/* the greatest similarity of the group under f32::total_cmp (bits, as matches.rs:28 compares) */
  uint32_t best_pattern;   /* least pattern_index among the group's records whose similarity has exactly those bits */
} fac_term;

/* Corpus totals (optional): a dense array of n_keys entries. count: the key's term counts summed
 * over the batch; docs: the documents that have a term of that key (the document frequency). */
typedef struct fac_term_total {
  uint64_t count;
  uint64_t docs;
} fac_term_total;

typedef struct fac_count_args {
  float threshold;
  int32_t order;               /* as fac_matches_apply */
  int32_t overlap;             /* as fac_matches_apply */
  const uint64_t* unique_ids;  /* as fac_matches_apply (host array, one key per pattern) */
  const uint32_t* keys;        /* host array, one key per pattern, or NULL (key = pattern index) */
  uint64_t n_keys;
  void* stream;
  void* device_out;            /* optional: terms stay in HBM */
  uint64_t device_cap;         /* in terms */
  uint64_t* device_doc_offsets; /* optional: n_docs+1 entries on the device, the CSR index into the terms */
  fac_term_total* device_totals; /* optional: n_keys entries on the device */
} fac_count_args;

/* Terms grouped by document, ascending document index, ascending key within a document. They go to
 * the host (*out, fac_buffer_free) or, with device_out set, into that device buffer of device_cap
 * terms (out may then be NULL); *n_out is the term count either way. doc_offsets (host array of
 * n_docs+1 entries, may be NULL) is the CSR index into the terms. totals (host array of n_keys
 * entries -- the engine's pattern count when keys == NULL -- may be NULL) receives the corpus totals;
 * when neither totals nor device_totals is given, nothing is launched or allocated for them.
 * FAC_E_OUTPUT_CAPACITY: device_cap is too small, *n_out holds the terms needed and nothing was
 * written to any device output (the counts are known before any term is written). */
int fac_count_batch(const fac_engine* engine, const fac_batch* batch, const fac_count_args* args, fac_term** out,
                    uint64_t* n_out, uint64_t* doc_offsets, fac_term_total* totals, fac_stats* stats);

/* fac_count_batch over fac_search_batch_prefiltered's search: the same relation as every other
 * _prefiltered pair, with its "all ASCII, or opted in" limit. */
int fac_count_batch_prefiltered(const fac_engine* engine, const fac_batch* batch, const fac_count_args* args,
                                fac_term** out, uint64_t* n_out, uint64_t* doc_offsets, fac_term_total* totals,
                                fac_stats* stats);

/* Tests and hosts: the rule above on the host for one document's n records (no device). keys: one
 * entry per pattern (n_patterns of them) or NULL, n_keys as above. Returns the term count, writing
 * the terms in ascending key order to out (cap terms; out == NULL: count only), or minus the error
 * code: FAC_E_INVALID for a key >= n_keys, a pattern_index >= n_patterns or a wrong n_keys with
 * keys == NULL; FAC_E_OUTPUT_CAPACITY (nothing written) when cap is too small; FAC_E_UNSUPPORTED for
 * n >= 2^32. */
int64_t fac_count_records(const fac_match* recs, uint64_t n, const uint32_t* keys, uint64_t n_patterns, uint64_t n_keys,
                          fac_term* out, uint64_t cap);

/* ---- Batched replace: FuzzyReplacer::replace (replacer.rs:22-25, query.rs:46-96,
 * matches.rs:165-188) of every document of a staged batch, spliced on the device.
 *
 * A replacement table gives each pattern its canonical form, or marks it "keep" (the callback's
 * None, matches.rs:180-183: the matched text stays). It is the per-pattern table FuzzyReplacer
 * uses (replacer.rs:24); a per-match callback cannot run on the device, but the callback the crate
 * documents, format!("**{}**", m.text) (matches.rs:445-446), is a template -- prefix + m.text +
 * suffix -- and those the table holds too (fac_replacements_create_templates below).
 * Replacement p is bytes [offsets[p], offsets[p+1]) of utf8 (offsets[0] == 0, non-decreasing,
 * empty = deletion), each valid UTF-8 on its own; keep: NULL, or one byte per pattern, non-zero = keep (its bytes are
 * ignored). Validated and uploaded once. FAC_E_INVALID: n_patterns differs from the engine's, bad
 * offsets or invalid UTF-8; FAC_E_UNSUPPORTED: 2^32 bytes of replacements or more. */
int fac_replacements_create(const fac_engine* engine, const uint8_t* utf8, const uint64_t* offsets,
                            const uint8_t* keep, uint64_t n_patterns, fac_replacements** out);
void fac_replacements_free(fac_replacements* replacements);

/* fac_replacements_create with template entries: the replacement of a match m of pattern p is
 * entry[..k] + m.text + entry[k..], the callback Some(format!("{pre}{}{suf}", m.text)) -- highlighting,
 * tagging, bracketing. insert_at: NULL (the call is fac_replacements_create), or one value per
 * pattern: FAC_NO_INSERT for a plain entry, or the byte position k in [0, len_p] the matched text goes
 * to, on a UTF-8 character boundary of entry p, so that both halves are valid UTF-8 on their own.
 * keep[p] != 0 wins over insert_at[p] as it wins over the bytes; an empty entry with k = 0 is "keep"
 * byte for byte. FAC_E_INVALID: k > len_p or k inside a character; everything else as
 * fac_replacements_create. The result is an ordinary table: fac_replace_batch,
 * fac_replace_batch_prefiltered and fac_extract_batch take it as they take any other, a skipped
 * record contributes nothing, template or not, and only a piece's length and bytes change. A table
 * without a template entry runs the same device code as one of fac_replacements_create. */
#define FAC_NO_INSERT UINT64_MAX
int fac_replacements_create_templates(const fac_engine* engine, const uint8_t* utf8, const uint64_t* offsets,
                                      const uint8_t* keep, const uint64_t* insert_at, uint64_t n_patterns,
                                      fac_replacements** out);

typedef struct fac_replace_args {
  float threshold;
  int32_t order;               /* as fac_matches_apply; 0 Unsorted is taken as 1 Default */
  int32_t overlap;             /* as fac_matches_apply; 0 Keep is taken as 1 NonOverlapping */
  const uint64_t* unique_ids;  /* as fac_batch_args */
  void* stream;
  void* device_out;            /* optional: the replaced bytes stay in HBM */
  uint64_t device_cap;         /* bytes device_out holds */
  uint64_t* device_out_offsets; /* optional: n_docs+1 entries on the device */
} fac_replace_args;

/* For every document d the result is engine.replace(doc_d, opts, callback) of the crate with
 * callback(m) = the table's entry for m.pattern_index. The options are normalised as `segmented`
 * does (query.rs:46-64; NonOverlappingUnique keeps its per-document used-pattern set), the batch is
 * searched and ranked as fac_search_batch does, and each document's kept records are walked in the
 * order fac_search_batch returns them -- by start, records of equal start in acceptance order --
 * with the loop of matches.rs:170-187: last = 0; a record with start >= last emits
 * doc[last..start], then its replacement (doc[start..end] for "keep"), and sets last = end; a
 * record with start < last is skipped; doc[last..] ends the document. Two kept records can share a
 * start (a span and the empty span at its start, or two empty spans, matches.rs:93-99); the crate
 * leaves their order open (sort_unstable_by_key, matches.rs:111), here it is the acceptance order
 * above. Offsets are byte offsets within the document, ASCII or not; the output is valid UTF-8.
 *
 * Output document d is bytes [out_offsets[d], out_offsets[d+1]) of the result; out_offsets is the
 * caller's host array of n_docs+1 entries (may be NULL). The bytes go to the host (*out,
 * fac_buffer_free) or, with device_out set, into that device buffer; *out_len is the byte count
 * either way and *n_replaced (may be NULL) the number of records the splice applied.
 * FAC_E_OUTPUT_CAPACITY: device_cap is too small, *out_len holds the bytes needed and nothing was
 * written. Errors and limits as fac_search_batch, and FAC_E_INVALID for a table of another pattern
 * count or device, FAC_E_UNSUPPORTED (never a partial result) for an output of 2^40 bytes or more. */
int fac_replace_batch(const fac_engine* engine, const fac_batch* batch, const fac_replacements* replacements,
                      const fac_replace_args* args, uint8_t** out, uint64_t* out_len, uint64_t* out_offsets,
                      uint64_t* n_replaced, fac_stats* stats);

/* fac_replace_batch over fac_search_batch_prefiltered's records: the same splice of
 * matches.rs:170-187, per document, of engine.with_prefilter().search(doc_d, opts) with the options
 * normalised as `segmented`. Arguments and contract as fac_replace_batch; fallback and limits as
 * fac_search_batch_prefiltered. */
int fac_replace_batch_prefiltered(const fac_engine* engine, const fac_batch* batch, const fac_replacements* replacements,
                                  const fac_replace_args* args, uint8_t** out, uint64_t* out_len, uint64_t* out_offsets,
                                  uint64_t* n_replaced, fac_stats* stats);

/* ---- Batched extraction: FuzzyMatches::matched_strings (matches.rs:513-515) of every document of
 * a staged batch, cut out on the device: a list-of-strings column, one string per kept record.
 *
 * For every document d, ms = engine.search(doc_d, opts) with the options exactly as passed (there is
 * no `segmented` normalisation: matched_strings works on whatever search returned). With table NULL
 * document d's items are ms.matched_strings(); with a table, item = callback(m), or m.text where the
 * callback gives None -- plain, "keep" and template entries all count (the canonical form of each
 * mention, say). Records and items are returned together and index the same: item i is the string
 * of record i, bytes [item_offsets[i], item_offsets[i+1]) of the text, and document d owns
 * [doc_offsets[d], doc_offsets[d+1]) of both. For Unsorted+Keep the order within a document is as
 * unspecified as fac_search_batch's; the pairing of record and item is not. Items may overlap in
 * the source (Overlap::Keep), so the text can exceed the batch, and may be empty. */
typedef struct fac_extract_args {
  float threshold;
  int32_t order;               /* as fac_matches_apply */
  int32_t overlap;             /* as fac_matches_apply */
  const uint64_t* unique_ids;  /* as fac_batch_args */
  void* stream;
  void* device_records;        /* optional: records stay in HBM (with device_text) */
  uint64_t device_record_cap;  /* records device_records holds */
  uint64_t* device_doc_offsets; /* optional: n_docs+1 entries on the device */
  void* device_text;           /* optional: the items' bytes stay in HBM (with device_records) */
  uint64_t device_text_cap;    /* bytes device_text holds */
  uint64_t* device_item_offsets; /* optional: device_record_cap+1 entries on the device */
} fac_extract_args;

/* doc_offsets: the caller's host array of n_docs+1 entries (may be NULL). Host results: *records
 * (fac_matches_free), *text and *item_offsets (*n_items + 1 entries; may be NULL), both
 * library-allocated and freed with fac_buffer_free. device_records and device_text are set together
 * or not at all (FAC_E_INVALID otherwise); then records and text go to those buffers,
 * device_item_offsets receives the first *n_items + 1 offsets, and records / text may be NULL.
 * *n_items and *text_len are the counts either way. FAC_E_OUTPUT_CAPACITY: either device buffer is
 * too small; nothing was written to either, and *n_items and *text_len hold what is needed.
 * FAC_E_INVALID for a table of another pattern count or device, FAC_E_UNSUPPORTED (never a partial
 * result) for 2^40 text bytes or more; other errors and limits, auto-beam and mapping engines as
 * fac_search_batch. */
int fac_extract_batch(const fac_engine* engine, const fac_batch* batch, const fac_replacements* table,
                      const fac_extract_args* args, fac_match** records, uint64_t* n_items, uint64_t* doc_offsets,
                      uint8_t** text, uint64_t* text_len, uint64_t** item_offsets, fac_stats* stats);

/* fac_extract_batch over fac_search_batch_prefiltered's records; fallback and limits as that call. */
int fac_extract_batch_prefiltered(const fac_engine* engine, const fac_batch* batch, const fac_replacements* table,
                                  const fac_extract_args* args, fac_match** records, uint64_t* n_items,
                                  uint64_t* doc_offsets, uint8_t** text, uint64_t* text_len, uint64_t** item_offsets,
                                  fac_stats* stats);

/* ---- Batched segmentation: segment_iter, split, strip_prefix, strip_suffix and segment_text
 * (query.rs:98-170, matches.rs:218-594) of every document of a staged batch, walked on the device.
 *
 * The options are normalised as `segmented` does (query.rs:46-64: 0 Unsorted is taken as 1 Default,
 * 0 Keep as 1 NonOverlapping; NonOverlappingUnique keeps its per-document used-pattern set), the
 * batch is searched and ranked as fac_search_batch does, and each document's kept records are
 * walked in the order fac_search_batch returns them -- by start, records of equal start in
 * acceptance order, as in fac_replace_batch -- with the loop of segment_iter (matches.rs:526-553):
 * last = 0; a record with start >= last emits Unmatched[last, start) if start > last, then
 * Matched(record), and sets last = end; a record with start < last is dropped; Unmatched[last, len)
 * ends the document if last < len. The segments tile [0, len). An unmatched segment is never empty;
 * a matched one is empty where the record's span is.
 *
 * A segment is a fac_match: a matched segment is the kept record verbatim, an unmatched one has its
 * start / end, pattern_index = FAC_UNMATCHED, similarity 0 and all counts 0. split (matches.rs:
 * 344-354) is the unmatched segments, in order. */
#define FAC_UNMATCHED 0xFFFFFFFFu

/* Segments grouped by document, offsets relative to the segment's own document; doc_offsets is the
 * CSR index into the segments. Arguments, contract, errors and limits are fac_search_batch's, with
 * device_out / device_cap counting segments, device_doc_offsets receiving the segment index, and
 * FAC_E_OUTPUT_CAPACITY (nothing written) reporting the segments needed in *n_out. */
int fac_segment_batch(const fac_engine* engine, const fac_batch* batch, const fac_batch_args* args, fac_match** out,
                      uint64_t* n_out, uint64_t* doc_offsets, fac_stats* stats);

/* fac_segment_batch over fac_search_batch_prefiltered's records; fallback and limits as that call. */
int fac_segment_batch_prefiltered(const fac_engine* engine, const fac_batch* batch, const fac_batch_args* args,
                                  fac_match** out, uint64_t* n_out, uint64_t* doc_offsets, fac_stats* stats);

/* The helpers that return a String, per document over the segments above:
 *   FAC_RENDER_STRIP_PREFIX  strip_prefix (matches.rs:218-245): doc[a..], a = the byte of the first
 *                            non-whitespace character of the first unmatched segment that has one;
 *                            empty if no unmatched segment has one.
 *   FAC_RENDER_STRIP_SUFFIX  strip_suffix (matches.rs:276-307): doc[..b], b = the end of the last
 *                            non-whitespace character of the last unmatched segment that has one;
 *                            empty if none has.
 *   FAC_RENDER_SEGMENT_TEXT  segment_text (matches.rs:566-594): the segments joined, with a U+0020
 *                            before a matched segment that follows a matched one or a result that
 *                            is not empty and does not end in U+0020 or U+0009, and before an
 *                            unmatched segment that follows a matched one unless it starts with one
 *                            of , . ? ! ; : U+2014 - U+2026.
 * Whitespace is Rust's char::is_whitespace (the Unicode White_Space property: U+0009-U+000D, U+0020,
 * U+0085, U+00A0, U+1680, U+2000-U+200A, U+2028, U+2029, U+202F, U+205F, U+3000); whitespace inside a
 * matched segment does not count. */
#define FAC_RENDER_STRIP_PREFIX 0
#define FAC_RENDER_STRIP_SUFFIX 1
#define FAC_RENDER_SEGMENT_TEXT 2

/* The output contract is fac_replace_batch's: document d is bytes [out_offsets[d], out_offsets[d+1])
 * of the result, on the host (*out, fac_buffer_free) or in args->device_out, with
 * args->device_out_offsets honoured; *out_len is the byte count either way; FAC_E_OUTPUT_CAPACITY:
 * device_cap is too small, *out_len holds the bytes needed and nothing was written. The output is
 * valid UTF-8. FAC_E_INVALID for a bad mode, FAC_E_UNSUPPORTED (never a partial result) for an output
 * of 2^40 bytes or more; errors and limits otherwise as fac_search_batch. */
int fac_render_batch(const fac_engine* engine, const fac_batch* batch, int32_t mode, const fac_replace_args* args,
                     uint8_t** out, uint64_t* out_len, uint64_t* out_offsets, fac_stats* stats);

/* fac_render_batch over fac_search_batch_prefiltered's records; fallback and limits as that call. */
int fac_render_batch_prefiltered(const fac_engine* engine, const fac_batch* batch, int32_t mode,
                                 const fac_replace_args* args, uint8_t** out, uint64_t* out_len, uint64_t* out_offsets,
                                 fac_stats* stats);

/* Streaming search (stream.rs:77-297): feed the input in the reader's read() pieces; windows
 * of `window_bytes` (0 = the crate's 256 KiB) are cut, searched (sorted + non-overlapping) and
 * their owned matches returned with absolute byte offsets, exactly like search_stream. Two windows
 * are searched at a time on two HIP streams (the next window's upload and search overlap the
 * current one's); matches are still returned in stream order. Each feed
 * returns the matches completed so far (`*out`, free with fac_matches_free) and their matched
 * bytes concatenated in the same order (`*text`, match i has end - start bytes; free with
 * fac_buffer_free). Pass eof = 1 (data may be empty) once the input has ended. */
typedef struct fac_stream fac_stream;
int fac_stream_open(const fac_engine* engine, float threshold, uint64_t window_bytes, fac_stream** out);
/* prefilter == 0: fac_stream_open. Otherwise every window is cut exactly as before and its text is
 * searched as engine.with_prefilter().search(text, sorted().non_overlapping()) (stream.rs:262-297
 * with Prefiltered::search, the semantics of fac_stream_window_staged(prefilter = 1)); ownership,
 * offsets and the output order do not change. Where the reference falls back to the full search (no
 * filter, or an edit budget over 24 at this threshold) the stream is the unfiltered stream. */
int fac_stream_open_ex(const fac_engine* engine, float threshold, uint64_t window_bytes, int32_t prefilter,
                       fac_stream** out);
/* The options form of the two calls above, and the one that takes the whole-token mask ("Whole-token
 * matches" above, the rule for a stream). FAC_E_INVALID for a NULL argument or a mask outside 0..3;
 * boundaries == 0 is fac_stream_open_ex. */
typedef struct fac_stream_options {
  float threshold;
  uint64_t window_bytes; /* 0 = the crate's 256 KiB */
  int32_t prefilter;     /* as fac_stream_open_ex */
  int32_t boundaries;    /* FAC_BOUNDARY_* mask, 0 = off */
} fac_stream_options;
int fac_stream_open_opts(const fac_engine* engine, const fac_stream_options* options, fac_stream** out);
/* Tests and hosts: the start windows of the segments handed to the search launcher, for the windows
 * handed out so far: the graphemes of every window's text for a plain stream (bytes where a window's
 * text is ASCII), the lengths of every window's merged bitap windows for a pre-filtered one. */
uint64_t fac_stream_windows_searched(const fac_stream* stream);
/* Tests and hosts: the device tasks of this stream handed out so far that were searched in one
 * pass (*batched: the ASCII union path or the window-documents path) and window by window
 * (*single). Either pointer may be NULL. */
void fac_stream_task_counts(const fac_stream* stream, uint64_t* batched, uint64_t* single);
int fac_stream_feed(fac_stream* stream, const uint8_t* data, uint64_t len, int32_t eof, fac_match** out,
                    uint64_t* n_out, uint8_t** text, uint64_t* text_len);
uint64_t fac_stream_total(const fac_stream* stream);
/* Commit point of the windows whose matches were handed out so far: every match still to come
 * starts at or after this offset (the streaming replace copies the text before it through). */
uint64_t fac_stream_committed(const fac_stream* stream);
void fac_stream_close(fac_stream* stream);
void fac_buffer_free(void* p);

/* Streaming replace against a replacement table: FuzzyReplacer::replace_stream (replacer.rs:35-44;
 * stream.rs:465-492 with ReplaceCursor::emit_window, :645-705) with callback(m) = the table's entry
 * for m.pattern_index. Windows are cut exactly as fac_stream_feed cuts them (64 KiB reads, the valid
 * UTF-8 prefix, the commit point at the overlap-th grapheme from the end, window growth;
 * stream.rs:102-158), so bytes after the last window's valid prefix are never written
 * (stream.rs:117-131). Each task of consecutive windows keeps its text on the device after the
 * search; its owned records are uploaded, the splice is planned and copied there
 * (fac_replace_windows_staged_device's kernels), and the output comes back. Two tasks are in flight:
 * their searches overlap, and a task's plan waits only for its predecessor's cursor. Each feed
 * returns the output completed so far (`*out`, *out_len bytes, fac_buffer_free), strictly in stream
 * order; pass eof = 1 (data may be empty) once the input has ended. The table must outlive the
 * stream. FAC_E_INVALID for a table of another pattern count or device; other errors as
 * fac_stream_feed. */
typedef struct fac_replace_stream fac_replace_stream;
int fac_replace_stream_open(const fac_engine* engine, const fac_replacements* replacements, float threshold,
                            uint64_t window_bytes, fac_replace_stream** out);
/* fac_replace_stream_open with fac_stream_open_ex's `prefilter`; the replace cursor does not change. */
int fac_replace_stream_open_ex(const fac_engine* engine, const fac_replacements* replacements, float threshold,
                               uint64_t window_bytes, int32_t prefilter, fac_replace_stream** out);
/* fac_replace_stream_open_ex with fac_stream_options (its whole-token mask included): only the set
 * of owned records changes; the splice, the cursor and its guard do not. */
int fac_replace_stream_open_opts(const fac_engine* engine, const fac_replacements* replacements,
                                 const fac_stream_options* options, fac_replace_stream** out);
uint64_t fac_replace_stream_windows_searched(const fac_replace_stream* stream);
/* fac_stream_task_counts of a replace stream. */
void fac_replace_stream_task_counts(const fac_replace_stream* stream, uint64_t* batched, uint64_t* single);
int fac_replace_stream_feed(fac_replace_stream* stream, const uint8_t* data, uint64_t len, int32_t eof, uint8_t** out,
                            uint64_t* out_len);
/* Bytes handed out so far: replace_stream's return value (ReplaceCursor::written) after the feed with eof. */
uint64_t fac_replace_stream_written(const fac_replace_stream* stream);
/* Records replaced, and records skipped because they start inside text an earlier window's match
 * already wrote (stream.rs:671-675), in the output handed out so far. Either pointer may be NULL. */
void fac_replace_stream_counts(const fac_replace_stream* stream, uint64_t* applied, uint64_t* skipped);
void fac_replace_stream_close(fac_replace_stream* stream);

/* Diagnostics: the merged candidate windows (grapheme ranges [start, end)) of the bitap
 * pre-filter for `threshold` (prefilter.rs:319-342). Returns the window count (writes up to `cap`
 * pairs into `out`), or -1 if the pre-filter would fall back to a full search. */
int64_t fac_prefilter_windows(const fac_engine* engine, const uint8_t* utf8, uint64_t len, float threshold,
                              uint64_t* out, uint64_t cap);

/* Engine introspection (tests / diagnostics). */
uint64_t fac_engine_num_nodes(const fac_engine* engine);
uint32_t fac_engine_max_edits_fast(const fac_engine* engine);

/* Host-side UTF-8 staging helpers exposed for tests: extended grapheme cluster segmentation
 * (UAX #29) and per-grapheme first-code-point folding. Writes up to `cap` entries. */
uint64_t fac_segment_graphemes(const uint8_t* utf8, uint64_t len, uint64_t* starts, uint64_t cap);
uint32_t fac_fold_first_char(const uint8_t* utf8, uint64_t len, int32_t case_insensitive);

/* Host-side builder helper exposed for tests: the order in which the reference iterates a trie
 * node's `transitions: FxHashMap<String, u32>` (builder.rs:336-342; FxHasher structs.rs:95-156 +
 * std's hashbrown) given the children's graphemes in insertion order (code points: grapheme i is
 * cps[off[i] .. off[i+1])). Writes the n insertion indices in iteration order to `order`. */
void fac_edge_order(const uint32_t* cps, const uint64_t* off, uint64_t n, uint32_t* order);

/* Diagnostics (tests): the device beam cut alone. Array a holds keys[offs[a] .. offs[a+1]) as the
 * penalties of a queue's pending states (2*bw < length <= 256 for lds == 1, <= 1024 for lds == 0;
 * lds == 2: a ring in global memory as on the largest HBM rung, length <= 2^20, count <= 16); the
 * kernel keeps bw of them exactly as the search's beam does -- the reference's
 * `queue[q_idx..].select_nth_unstable_by(bw - 1, total_cmp)` + `truncate(q_idx + bw)`
 * (search.rs:584-587) -- and writes the survivors' original indices, in queue order, to
 * perm[a*bw .. a*bw + bw). sel_limit < 0: core's 16 partition rounds. Uses device 0. */
int fac_diag_beam_select(const float* keys, const uint64_t* offs, uint64_t count, uint32_t bw, int32_t lds,
                         int32_t sel_limit, uint32_t* perm);

/* Diagnostics (tests): the device reduce of fac_count_batch alone, with no engine and no search.
 * recs: n records grouped by document, document d's being recs[doc_offsets[d] .. doc_offsets[d+1])
 * (n_docs + 1 ascending offsets from 0 to n, n_docs <= 2^24); only pattern_index (< n_patterns) and
 * similarity are read. keys, n_keys: as fac_count_records. lane_max, group_max: the greatest record
 * counts a document may have to be grouped by one lane / by one workgroup (0: the library's
 * defaults, 8 and 2048; above them: FAC_E_INVALID); larger documents go through the device sort.
 * The terms come back in *out (fac_buffer_free) with *n_out, term_offsets (n_docs + 1 entries) and
 * totals (n_keys entries -- n_patterns when keys == NULL; may be NULL: nothing runs for them). Uses device 0. */
int fac_diag_count_terms(const fac_match* recs, uint64_t n, const uint64_t* doc_offsets, uint64_t n_docs,
                         const uint32_t* keys, uint64_t n_patterns, uint64_t n_keys, uint32_t lane_max, uint32_t group_max,
                         fac_term** out, uint64_t* n_out, uint64_t* term_offsets, fac_term_total* totals);

/* Diagnostics (tests): what a search does with its engine's snapshot store, from the store's host state
 * alone (no device): 0 carries over, else the reason it starts the store empty (1 fresh, 2 signature,
 * 3 pool, 4 directory) or does without it (5 busy: another call holds it; busy != 0 holds the store's
 * lock while a second thread takes the call's steps; 7 gated: sleep != 0). calls: the calls the store has served since it was
 * last empty; used, cap, last_call (appended by the previous call), want_cap (what this call would
 * allocate), cap_limit: pool words; pending: a reason the previous call left. Signatures are 16 words,
 * the directory arrays 9 entries (by key length). fac_diag_rc_reset_name: the reason as the
 * FAC_RC_DEBUG line prints it. */
int fac_diag_rc_store_decide(int32_t valid, uint64_t calls, uint64_t used, uint64_t cap, uint64_t last_call,
                             int32_t pending, const uint32_t* have_sig, const uint32_t* want_sig, uint64_t want_cap,
                             uint64_t cap_limit, const uint64_t* dir_slots, const uint64_t* dir_keys, int32_t busy,
                             uint32_t sleep);
const char* fac_diag_rc_reset_name(int32_t reset);
/* The store's gate for unlike text: the calls that go without the store (7 gated; `sleep` above) after a
 * carrying call that found `carried` of its carried + built entries: 0 from a tenth on or below gate_min
 * entries, else twice `backoff` (1 at first, at most 64). */
uint32_t fac_diag_rc_store_gate(uint64_t carried, uint64_t built, uint32_t backoff, uint64_t gate_min);
/* The gate for a store that every call empties (fresh-word text fills the pool in one call): the calls
 * that go without the store, the deciding one included, when `decision` (fac_diag_rc_store_decide) is
 * 3 pool or 4 directory right after the call that filled the store from empty (after_fill != 0): twice
 * `backoff` (1 at first, at most 64); 0: the rule does not apply. */
uint32_t fac_diag_rc_emptied_gate(int32_t decision, int32_t after_fill, uint32_t backoff);
/* Whether a call searches from the store's directories alone: unknown_pm per mille of its `sampled`
 * windows ended on a key no directory holds; floor_pm: the share the last full call left (< 0: none);
 * 1 when unknown_pm <= floor_pm + margin_pm, sampled > 0 and windows >= min_windows. */
int32_t fac_diag_rc_direct_decide(uint32_t unknown_pm, int32_t floor_pm, uint32_t margin_pm, uint64_t sampled,
                                  uint64_t windows, uint64_t min_windows);

/* Diagnostics (tests): the expanded text of a stream task alone. Window w is bytes
 * [windows[2w], windows[2w] + windows[2w + 1]) of the len bytes at utf8 (ranges may overlap); the
 * device copies them one after the other into `out` (cap bytes; the lengths summed must fit) and
 * writes the n_windows + 1 document offsets to `offsets`. FAC_E_INVALID for a range outside the
 * text. Uses the engine's device. */
int fac_diag_stream_gather(const fac_engine* engine, const uint8_t* utf8, uint64_t len, const uint64_t* windows,
                           uint64_t n_windows, uint8_t* out, uint64_t cap, uint64_t* offsets);

#ifdef __cplusplus
}
#endif

#endif /* FAC_H */
