// common.h -- context object and helpers shared by the stage implementations of libbcehip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <exception>
#include <new>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include <sys/mman.h>

#include "../../include/bce_hip.h"
#include "bce_core.h"
#include "host_coder.h"

namespace bce {

// grow-only device buffer
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

// Device-resident control block of the enumeration (K3).  Everything a round needs to know about
// the previous round lives here, so rounds can be queued back to back without host round trips.
struct EnumCtl {
  uint32_t cnt[2][8][2];     // [parity][plane][seg] node counts (seg0 = child0 list, seg1 = child1 list)
  uint64_t sym_total;        // symbol records in the buffer (since the last flush)
  uint64_t sym_cap;          // capacity of the symbol buffer
  uint64_t nodes_total;      // nodes visited so far
  uint32_t need_flush;       // a round was skipped because the symbol buffer could overflow
  uint32_t skip_round;       // first skipped round
  uint32_t done_round;       // first round whose successor is empty (0xFFFFFFFF while running)
  uint32_t overflow;         // node buffer overflow (fatal)
  uint64_t next_nodes;       // node total of the next round (after the last executed round): up to 8 (n/2) = 2^33
  uint64_t want_syms;        // symbol records of the skipped round (to grow the buffer when one round exceeds it)
  uint32_t ticket;           // k3_scan_kernel: arrival counter of its 8 plane blocks (last one runs the epilogue)
  uint32_t pad1;
  uint32_t ptot[8][3];       // per plane totals of the round: child0, child1, symbols
  uint64_t symbase[8];       // symbol-buffer base of each plane's records in this round
  uint32_t tail_rounds;      // rounds executed by the last k3_tail_kernel launch
  uint32_t small_bail;       // k3_small_kernel: the round (skip_round) does not fit its grid / tile table: run it wide
  uint32_t want_list;        // with `overflow`: the longest list the skipped round would write (the host makes that room: k3_grow_lists)
  uint32_t stalled;          // a single-launch round waited K3_SPIN_LIMIT polls for a predecessor tile's word: fatal, loud (see wait_word)
};

// Pinned host staging of one model flush + the batch descriptor handed to the coder threads.
struct FlushSlot {
  uint64_t *h_out = nullptr;     // one packed u64 per symbol (bce_core.h pack_model_out)
  size_t cap = 0;
  CoderBatch batch;
  hipEvent_t ev_start = nullptr, ev_copy = nullptr;   // K4 start (compute stream), outputs in h_out (copy stream)
  hipEvent_t ev_kend = nullptr;                       // K4's last kernel (compute stream): the kernels' own time, without the copy
  bool timed = false;            // the events of the last flush have not been added to stats.t_model yet
  std::shared_ptr<std::once_flag> once;   // the first coder thread to arrive waits for ev_copy, the others for it
  bool registered = false;       // h_out is a private mapping under hipHostRegister (k4_prepin), not hipHostMalloc's
  // staged ahead of its first use, on a thread of its own (k4_prepin): the buffer it prepares, adopted by the next flush
  std::thread pin_th;
  uint64_t *pin_p = nullptr;
  size_t pin_cap = 0;
  double pin_s = 0;
  // estimate mode (k4_cost.hip): the flush's run table on its way to the device, pinned; free again once ev_copy has fired
  void *h_cost_runs = nullptr;
  size_t h_cost_runs_cap = 0;
};

// ---- host memory registered with the runtime (hipHostRegister) ------------------------------------------------------------
// Rules, each closing one way in which a registered range can lose its pages under the GPU (round 4's
// "memory access fault ... write access to a read-only page" at an address inside the C library's heap):
//  1. A registered range is ALWAYS an anonymous private mapping of its own (huge_map) -- never memory carved out of the C
//     library's heap, whose pages go back to the kernel (brk trim), to other callers and to khugepaged as malloc sees fit.
//  2. MADV_DONTFORK: a fork() of the host program (Python's subprocess, system()) does not turn the pages copy-on-write under
//     the device's mapping (what the runtime's own pinned memory has).
//  3. Huge pages are taken at the FIRST TOUCH only: the caller touches every page (reg_map_settle), then the mapping is
//     MADV_NOHUGEPAGE -- the huge pages it got stay, but khugepaged never collapses 4 KB pages into a new huge page (= other
//     physical pages) while the range is registered.
//  4. hipHostUnregister does not wait for the device (hipHostFree does): before it, the owner waits for exactly the events /
//     streams whose work touches the range (the slot's copy event; the context's three streams) -- not hipDeviceSynchronize,
//     which would stall the other contexts of a pool.
// BCE_HIP_REG_MIN=bytes lowers the sizes from which buffers take this route (defaults: 8 MB for a flush slot, 256 MB for the
// decoder's boundary ranks) so that tests reach it with small inputs.
inline size_t reg_min_bytes(size_t dflt) {
  const char *e = getenv("BCE_HIP_REG_MIN");                          // (read per allocation: a test sets it for one context)
  return e ? (size_t)strtoull(e, nullptr, 10) : dflt;
}
// An anonymous mapping of its own, 2 MB-aligned, with huge pages asked for (3.2 GB are touched in a tenth of the time; the coder
// threads that read the staging buffers gain 1-2 %): `bytes` usable at the returned
// address; huge_unmap gives it back.  (The mapping is 2 MB longer than asked; the unaligned head and tail go back at once.)
inline void *huge_map(size_t bytes) {
  const size_t two_mb = (size_t)2 << 20, used = (bytes + 4095) & ~(size_t)4095;
  void *base = mmap(nullptr, used + two_mb, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
  if (base == MAP_FAILED) return nullptr;
  char *q = reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(base) + two_mb - 1) & ~(uintptr_t)(two_mb - 1));
  const size_t head = (size_t)(q - static_cast<char *>(base));          // (a multiple of the page size, below 2 MB)
  if (head) (void)munmap(base, head);                                    // what lies in front of the aligned address ...
  if (two_mb - head) (void)munmap(q + used, two_mb - head);              // ... and behind the end goes back at once
  (void)madvise(q, used, MADV_DONTFORK);                                 // rule 2
  static const bool no_thp = getenv("BCE_HIP_NO_THP") != nullptr;     // (diagnostic: what a host without free huge pages gives)
  if (!no_thp) (void)madvise(q, used, MADV_HUGEPAGE);
  return q;
}
// every page of the mapping has been touched: from here on its physical pages stay what they are (rule 3)
inline void reg_map_settle(void *q, size_t bytes) { (void)madvise(q, (bytes + 4095) & ~(size_t)4095, MADV_NOHUGEPAGE); }
inline void huge_unmap(void *q, size_t bytes) { if (q) (void)munmap(q, (bytes + 4095) & ~(size_t)4095); }
// bytes of the mapping k4_prepin makes for a slot of `cap` records
inline size_t slot_map_bytes(size_t cap) { return (cap * 8 + 16 + 4095) & ~(size_t)4095; }
// free a slot's host staging, whichever way it was pinned.  The only device work that touches a slot's staging is the
// device-to-host copy of its last flush, which ev_copy follows (rule 4; an event never recorded is complete).
inline void slot_free_host(FlushSlot &s, uint32_t *unmaps = nullptr) {
  if (s.h_out) {
    if (s.registered) {
      if (s.ev_copy) (void)hipEventSynchronize(s.ev_copy);
      (void)hipHostUnregister(s.h_out);
      huge_unmap(s.h_out, slot_map_bytes(s.cap));
      if (unmaps) ++*unmaps;
    } else (void)hipHostFree(s.h_out);
  }
  s.h_out = nullptr; s.cap = 0; s.registered = false;
}

struct RunEntry { uint64_t start; uint32_t count; uint32_t round; };  // symbols of (round, plane): [start, start+count)

// The buffers of the index queries (bce_hip_ctx::qbuf[qb::name], kd_count / _locate / _match / _lcp / _parse / _self.hip and api_index.hip):
// one array, so that bce_hip_destroy releases them in one loop and a name added here needs nothing else.
namespace qb {
enum Id {
  cnt_res,                                       // kd_count.hip: its flag word (a buffer of its own, as cmp_res)
  cnt_pat, cnt_off, cnt_out,                     // bce_hip_count: the patterns, their offsets and the counts of a call with host buffers, staged (grow-only)
  loc_res,                                       // kd_locate.hip: its flag word and scan total (a buffer of its own, as cnt_res)
  loc_lo, loc_cnt, loc_drop, loc_start, loc_lin, loc_bsum,   // per pattern: the interval's first row, its rows, those across the text's end; the two CSR offset arrays; the scan's block sums
  loc_key0, loc_key1, loc_val0, loc_val1,        // (position, pattern) of every row: both halves of the sorts' ping-pong
  loc_pat, loc_off, loc_hits, loc_pos,           // bce_hip_locate: the arrays of a call with host buffers, staged (all grow-only)
  near_res,                                      // kd_near.hip: its flag word (a buffer of its own, as loc_res); its scratch is the locate's loc_cnt .. loc_val1
  near_pat, near_off, near_out,                  // bce_hip_count_near / _locate_near: the patterns, their offsets and the counts of a call with host buffers, staged (grow-only)
  near_hits, near_pos, near_dist,                // bce_hip_locate_near with host buffers: the CSR offsets, positions and distances, staged (grow-only)
  cls_res,                                       // kd_classes.hip: its flag word (a buffer of its own, as near_res); its locate's scratch is loc_cnt .. loc_val1
  cls_kind, cls_pat,                             // the prepare pass: 16 bits per class of the batch (class_summary), two words per pattern (wide classes, the leftmost)
  cls_mask, cls_off, cls_out, cls_work, cls_status,   // bce_hip_count_classes / _locate_classes: masks, offsets, counts, nodes and verdicts of a call with host buffers, staged (grow-only)
  cls_hits, cls_pos,                             // bce_hip_locate_classes with host buffers: the CSR offsets and positions, staged (grow-only)
  mat_res,                                       // kd_match.hip: the coverage's result word (a buffer of its own, as loc_res)
  mat_bsum,                                      // the coverage scan's block maxima and block counts
  mat_qry, mat_len, mat_pos,                     // bce_hip_match / _coverage: the query of a call with a host buffer, the lengths and the positions, staged (all grow-only)
  rep_res,                                       // kd_lcp.hip: its result words, up to 64 k-gram records or the longest repeat's three (a buffer of its own, as mat_res)
  rep_bsum,                                      // the class and repeat reductions' per-block parts and maxima
  rep_lcp,                                       // the LCP array of a call that does not bring device memory for it: n words (grow-only, never kept as a cache)
  top_res,                                       // kd_lcp.hip, the most frequent k-grams: the 32 counters of the size histogram (a buffer of its own, as rep_res)
  top_bsum,                                      // per block: its candidates (then their offsets), its class-start carry, its 32 counters
  top_key0, top_key1, top_val0, top_val1,        // (key_max - size, first row) of every candidate: both halves of the sort's ping-pong, sized by the histogram's count
  top_out, top_bytes,                            // bce_hip_top_kgrams with host buffers, and the hook: the entries and the k-grams' bytes, staged (all grow-only)
  par_res,                                       // kd_parse.hip: the result words of the parse and of the patch (a buffer of its own, as mat_res)
  par_exit, par_entry, par_flag,                 // the parse: every position's exit from its block (+ 1), the blocks' entries, the flag byte per position
  par_bsum, par_bcnt,                            // the blocks' sums (parse: heads and literals packed; patch: lengths, literal lengths) and their counts / flag bits
  par_hpre,                                      // per op head: the literal bytes up to it
  par_off, par_loff,                             // the patch: every op's offset in the output and in the literal bytes
  par_ops, par_lits, par_out,                    // bce_hip_parse / _patch with host buffers: the ops, the literal bytes and the result, staged (all grow-only)
  slf_tree, slf_top,                             // kd_self.hip: the blocks' min-trees (2048 words a block) and the tree over the blocks' minima
  slf_rlen, slf_rsrc, slf_rtext,                 // the self-parse: lpf, src and the text written at n - 1 - i, what kd_parse's chain runs on
  slf_lpf, slf_src, slf_ops, slf_lits,           // bce_hip_lpf / _self_parse with host buffers: the arrays, the ops and the literal bytes, staged (all grow-only)
  mxr_res,                                       // kd_maxrep.hip: the 64 weight counters, the capped count and the BWT's change count (a buffer of its own, as top_res)
  mxr_bsum,                                      // per block: its changes / candidates (then their offsets) and its 65 counters
  mxr_chg, mxr_wt, mxr_first,                    // per row: the changes up to it (4 bytes), the weight it represents or 0 (8), that interval's first row (4)
  mxr_lo0, mxr_lo1, mxr_hi0, mxr_hi1, mxr_val0, mxr_val1,   // (complement of the weight, representative row) of every candidate: the sort's ping-pong, sized by the histogram's count
  mxr_out, mxr_bytes,                            // bce_hip_maximal_repeats with host buffers, and the hook: the entries and the repeats' bytes, staged (grow-only)
  sfc_res,                                       // kd_sufsort.hip: the checker's three result words (a buffer of its own, as par_res)
  sfc_inv, sfc_bsum,                             // the checker's inverse (n words) and the three stages' block results
  sfc_text, sfc_sa,                              // bce_hip_sufcheck with host buffers: the text and the array, staged (grow-only)
  sfa_sa, sfa_isa,                               // bce_hip_suffix_array with host buffers: the array and its inverse, staged (grow-only)
  edit_res,                                      // kd_edit.hip: its flag word (a buffer of its own, as near_res); its scratch is the locate's loc_res .. loc_val1
  edit_cnt,                                      // the reduce: every pattern's hits, what the scan turns into hit_offsets
  edit_pat, edit_off, edit_out,                  // bce_hip_count_edit / _locate_edit: the patterns, their offsets and the counts of a call with host buffers, staged (grow-only)
  edit_hits, edit_pos, edit_len, edit_dist,      // bce_hip_locate_edit with host buffers: the CSR offsets, positions, lengths and distances, staged (grow-only)
  count
};
}  // namespace qb

}  // namespace bce

struct bce_hip_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t copy_stream = nullptr;             // device-to-host copies of the model outputs, overlapping the next rounds
  // K4 (model flushes) on a stream of its own, lowest priority: the next K3 rounds run beside it.  K3 writes its symbol
  // records into skey[0] / sesc, K4 reads the pair of the flush before (skey_alt / sesc_alt): the two are swapped at
  // every flush.  Off by default (BCE_HIP_OVERLAP=1 or debug knob 11 switch it on): see bce_hip_create.
  hipStream_t k4_stream = nullptr;
  hipEvent_t ev_k3_batch = nullptr;              // the rounds whose symbols a flush takes are done (main stream)
  hipEvent_t ev_k4_done[2] = {nullptr, nullptr}; // flush f's kernels have read their symbol buffers (k4 stream), f & 1
  bool overlap = false;
  bool gated = true;                             // bce_hip_set_gated: the enumerations of one device's contexts take turns (default on)
  bool gate_held = false;
  bool gate_lent = false;                        // given to a waiting context behind a model flush (api.hip: gate_lend / gate_regain)
  double gate_t0 = 0, gate_wait_s = 0, gate_held_s = 0;   // (BCE_HIP_GATE_TIMING: seconds this compression waited for / held the device gate)
  uint32_t flush_seq = 0;                        // flushes issued by this context (parity selects ev_k4_done)
  hipEvent_t copy_busy = nullptr;                // last copy out of `sout` (the next K4 must not overwrite it earlier)
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_k4 = nullptr;
  char err[256] = {0};

  uint32_t n = 0;
  int stage = 0;  // 0 empty, 1 loaded, 2 bwt, 3 planes, 4 encoded
  int phase = 0;  // what is running: 1 K1, 2 K2, 3 the enumeration / model (-c, -s), 4 a decode, 5 the inverse BWT of the libdivsufsort
                  // seam (bce_hip_inverse_bwt), 6 the early rounds of the enumeration with K1 unfinished, K1's second half and the
                  // second plane build of a one-shot compression (K1's, K2's and K3's buffers are all live);
                  // 0 nothing.  Every entry point that sets it sets it back to 0.  ctx_trim() gives back the
                  // buffers the running phase does not use when the device runs out of memory (the context keeps every stage's
                  // buffers for its next input; at n ~ 2^31 they do not all fit together)
  uint32_t offset = 0;
  uint8_t config[9][32];
  bce::PlaneCfg cfg[8];
  uint32_t zeros[8] = {0};
  bool k1_unique = false;                        // K1 ended with all rotations distinct
  bool k1_valid = false;                         // sa[sa_res] / rank hold this input's suffix order (K1 ran; no injected BWT)
  int sa_res = 0;
  // K1 in two halves (k1_first_sort / k1_finish): which of sa[] / key[] / khi[] holds the first sort's result, the bytes of a
  // rotation it has ordered, and whether that order was the final one already.  k1_carry: the sorted keys hold each rotation's
  // preceding byte in their low 8 bits (the provisional BWT is read off them; k1_finish masks it out)
  int k1_res = 0;
  uint32_t k1_h = 0;
  bool k1_first_final = false;
  bool k1_carry = false;
  uint32_t k1_h_asked = 0;                       // the depth the caller's table asked for (k1_h: what it got, after the overrides)
  uint64_t plane_syms[8] = {0};                  // symbol records handed to each plane's coder since encode_start
  // debug knobs (bce_hip_debug_set): 0 = default
  uint32_t dbg_dfs_budget = 0, dbg_no_dfs = 0, dbg_no_tail = 0, dbg_no_skip = 0, dbg_no_small = 0, dbg_step_small = 0, dbg_no_fused = 0, dbg_no_local = 0, dbg_capp_div = 0, dbg_local_from = 0, dbg_local_budget = 0, dbg_tail_round = 0;
  uint32_t dbg_dec_budget = 0;                   // knob 13: the decoder's query budget (0 = 2^30)
  uint32_t dbg_oom = 0;                          // knob 14: allocations that fail for real (common.h: test_oom_fails)
  uint64_t sym_cap_user = 0;
  bool sync_flush = false;                       // BCE_HIP_SYNC_FLUSH: flushes wait for their copy (profiling)
  bce_hip_progress_fn progress = nullptr;        // bce_hip_set_progress
  void *progress_user = nullptr;

  // device buffers (grow-only)
  bce::DevBuf text, bwt;                         // n bytes each
  bce::DevBuf sa[2], key[2], rank, k2, nrk, act[2];   // K1: 9 x 4n (act = active-set lists)
  bce::DevBuf khi[2], dl[4], kflag, actv[2];                   // K1: high key words of the first sort, then new rank / suffix per active element;
                                                      //     deferred (big-group) lists; per-element flags
  bce::DevBuf rs_hist, blk;                      // radix histograms [256][nb]; per-block scratch
  bce::DevBuf ptmp[2];                           // K2 byte ping-pong
  bce::DevBuf gran;                              // 8 planes x ngran x 16 B
  uint32_t ngran = 0;                            // granules per plane
  // node lists: one buffer per round parity, 8 planes x capL[parity] nodes each (a round reads one parity and writes the
  // other; the one about to be written holds nothing and can be replaced by a larger one without a copy: k3_grow_lists).
  bce::DevBuf nlist[2];
  uint32_t capL[2] = {0, 0};
  // The decoder's node lists: one buffer per (parity, plane).  In a round only plane p writes plane p + 1's list of the other
  // parity, so a list that is too small for a plane's children is replaced alone (kd_decode.hip).
  bce::DevBuf dlist[2][8];
  int dec_part = 0;                              // of a decode (phase 4): 1 the rounds, 2 planes and unbwt, 3 the inverse BWT
  bce::DevBuf ctl, tilecnt, tileoff, runs;       // K3 control
  bce::DevBuf smwords;                           // k3_small_kernel: one published count word per tile
  size_t k3_groups = 0;
  uint32_t k3_count2_grid = 0;                   // blocks of k3_count2_kernel that are resident together
  bce::DevBuf k3tw, k3grp;                       // k3_count2_kernel: count word per tile; group words, tickets, offsets
  bce::DevBuf dfs;                               // depth-first tail: tagged symbols, sort scratch, walker stacks
  bce::DevBuf truns;                             // run table of the persistent tail kernel [K3_TAIL_MAXROUNDS][8]
  void *h_truns = nullptr;
  bce::DevBuf skey[2], sval[2], sout, sesc;       // K3->K4: symbol keys (skey[0]) + escape words (sesc); sort ping-pong; outputs
  bce::DevBuf skey_alt, sesc_alt, rs_hist_k4;     // the other pair of symbol buffers (see k4_stream); K4's radix histograms
  uint64_t sym_cap = 0;
  bool estimate_mode = false;                    // bce_hip_estimate is running: every plane's symbols are recorded, whatever the coder's plane mask
  bool scan_mode = false;                        // `bce -s`: K3 emits scan_pack words (bce_core.h) into scanrec
  bce::DevBuf scanrec;
  bce::DevBuf stat, dcfg, k4w;                   // K4 counters, device copy of PlaneCfg[8], per-window work arrays
  bce::DevBuf cost_acc, cost_runs;               // k4_cost.hip: eight cost sums + eight record counts; the run table of the flush being summed
  bce::DevBuf crc_tab;                           // kd_crc32.hip: the step tables of a launch of crc_tab_grid workgroups, its constants, its result word
  uint32_t crc_tab_grid = 0;                     // 0: no step tables uploaded
  bce::DevBuf cmp_res;                           // kd_compare.hip: its result word (a buffer of its own, as kd_crc32.hip's: no stage's scratch is touched)
  bce::DevBuf qbuf[bce::qb::count];              // the index queries' buffers, one per bce::qb name (above): each its own grow-only allocation
  bce::DevBuf hook[3];                           // test hooks bce_hip_sort_pairs_device / _wide_device: the second halves of the sorts' ping-pong
  bool crc_const_ready = false;                  // its launch-independent constants are uploaded
  bool text_loaded = false;                      // `text` holds the n bytes of the last bce_hip_load_* (bce_hip_input_crc32)
  uint32_t stat_off[8] = {0};
  bool model_hook = false;                       // bce_hip_model_begin ran: bce_hip_model_flush may follow

  // pinned host staging
  void *h_ctl = nullptr, *h_runs = nullptr;
  void *h_small = nullptr;                       // 4 KB of pinned host memory for read_back()
  void *h_big = nullptr;                         // pinned host memory for the decoder's host tail (the boundary ranks: 32 (n + 1) bytes), grow-only
  size_t h_big_cap = 0;
  uint32_t dec_restarts = 0;                     // (no decode starts again since the lists grow in place: stays 0)
  uint64_t dec_list_grows = 0, dec_split_rounds = 0;
  uint32_t reg_maps = 0, reg_unmaps = 0;         // registered host mappings made / given back since the context was created
  bool h_big_registered = false;                 // h_big is big_host_alloc's private mapping under hipHostRegister
  void *dec_pin[3] = {nullptr, nullptr, nullptr};  // the decoder's pinned query / escape-record / answer buffers, kept from one decode to the next (grow-only)
  size_t dec_pin_cap[3] = {0, 0, 0};
  bce::FlushSlot slot[3];                        // flushes in flight: GPU fills one while the coders drain the others
  int slot_next = 0;

  // enumeration stepping state
  uint32_t round = 0;
  bool enum_active = false;
  std::vector<bce::RunEntry> run_log[8];         // runs since the last flush, per plane

  bce::HostCoder *coder = nullptr;
  bce_hip_stats stats;
  // where a cold context's time goes (BCE_CLI_TIMING=1 prints them): device allocations, pinned host allocations
  // k4_prepin's threads touch their pages at once and register them with the runtime when it is up (bce_hip_create_sized
  // starts them BEFORE the runtime's initialisation): 0 = wait, 1 = go, 2 = give up
  std::mutex stage_mu;
  std::condition_variable stage_cv;
  int stage_state = 1;
  double alloc_s = 0, pin_s = 0;
  uint64_t alloc_bytes = 0, pin_bytes = 0;
  uint32_t alloc_calls = 0, pin_calls = 0;
};

namespace bce {

inline double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// The decoder's large pinned host buffer (the boundary ranks of the host tail: 32 (n + 1) bytes, 3.2 GB at 10^8): from 256 MB on
// (reg_min_bytes), a private mapping (huge_map), touched by four threads, then registered with the runtime (hipHostRegister,
// mapped: the device address is the host's, or the buffer is given up).  Measured: 3.2 GB in 0.04 s against
// hipHostMalloc's 0.55-0.7 s, which also holds the kernels queued meanwhile up.  Only the copy engine and the host touch this
// buffer.  The small buffers KERNELS write while the host reads (queries, answers, the mailbox) are hipHostMalloc's.
// BCE_DEC_NO_HUGE=1: hipHostMalloc for all.  big_host_free waits for the owning context's streams first (rule 4 above).
void *big_host_alloc(size_t bytes, int device, bool *registered);
void big_host_free(bce_hip_ctx *c, void *p, size_t bytes, bool registered);

inline int set_err(bce_hip_ctx *c, hipError_t e, const char *what, int line) {
  snprintf(c->err, sizeof c->err, "%s:%d: %s", what, line, hipGetErrorString(e));
  return e == hipErrorOutOfMemory ? BCE_HIP_E_NOMEM : BCE_HIP_E_DEVICE;
}

#define BCE_HIP_TRY(ctx, expr)                                        \
  do {                                                                \
    hipError_t _e = (expr);                                           \
    if (_e != hipSuccess) return bce::set_err((ctx), _e, #expr, __LINE__); \
  } while (0)

#define BCE_TRY(expr)                 \
  do {                                \
    int _rc = (expr);                 \
    if (_rc != BCE_HIP_OK) return _rc; \
  } while (0)

size_t ctx_trim(bce_hip_ctx *c);                   // api.hip: bytes given back (0: nothing left to give)
// BCE_HIP_TEST_OOM=k (test hook): every k-th device allocation of the process is treated as "out of memory" at its first attempt,
// so that the give-back-and-retry path runs in every phase without a 288 GB input.
inline bool test_oom_now() {
  static const char *e = getenv("BCE_HIP_TEST_OOM");
  static const unsigned long k = e ? strtoul(e, nullptr, 10) : 0;
  static std::atomic<unsigned long> count{0};
  return k && (count.fetch_add(1) + 1) % k == 0;
}
// What an allocation is, for test knob 14: a node list's growth at its first-choice size, or at the size it falls back to when
// that one does not fit (k3_grow_lists; the decoder's grow_lists), or anything else.
enum AllocSite { kAllocPlain = 0, kAllocListFirst = 1, kAllocListFallback = 2 };
// Test knob 14 (bce_hip_debug_set), per context, 0 = off: which attempts of ensure() fail -- for real, not pretended: hipMalloc is
// asked for more than the device holds (hipMemGetInfo's total + 1 GiB), so the error is the runtime's own and stays set until it is
// read, exactly as on a full device.  1 = both attempts at a node list's first-choice size (its fallback size succeeds), 2 = every
// attempt of a node list's growth, 3 = the first attempt of every allocation (the second, after ctx_trim, asks for the real size).
inline bool test_oom_fails(const bce_hip_ctx *c, int site, int attempt) {
  switch (c->dbg_oom) {
    case 1: return site == kAllocListFirst;
    case 2: return site != kAllocPlain;
    case 3: return attempt == 0;
    default: return false;
  }
}
inline size_t test_oom_bytes(size_t bytes) {
  size_t fr = 0, tot = 0;
  if (hipMemGetInfo(&fr, &tot) != hipSuccess) { (void)hipGetLastError(); return bytes; }
  return tot + ((size_t)1 << 30);
}
inline int ensure(bce_hip_ctx *c, DevBuf &b, size_t bytes, int site = kAllocPlain) {
  if (bytes <= b.cap) return BCE_HIP_OK;
  if (b.p) {
    // The old buffer may still be read or written by work this context has queued (a model flush and its copy run
    // behind the host): nothing of it may be in flight when the memory goes back to the allocator, because another
    // context's hipMalloc -- another host thread -- can be handed it at once.
    for (hipStream_t st : {c->stream, c->k4_stream, c->copy_stream}) if (st) BCE_HIP_TRY(c, hipStreamSynchronize(st));
    (void)hipFree(b.p);
    b.p = nullptr; b.cap = 0;
  }
  const double t0 = now_s();
  const bool hooked = c->dbg_oom != 0;
  hipError_t e = hipMalloc(&b.p, test_oom_fails(c, site, 0) ? test_oom_bytes(bytes) : bytes);
  const bool pretend = e == hipSuccess && test_oom_now();
  if (pretend) { (void)hipFree(b.p); e = hipErrorOutOfMemory; }
  if (e == hipErrorOutOfMemory) {
    // the buffers of the stages that are not running go back, then once more
    (void)hipGetLastError();
    b.p = nullptr;
    if (ctx_trim(c) || pretend || hooked) e = hipMalloc(&b.p, test_oom_fails(c, site, 1) ? test_oom_bytes(bytes) : bytes);
  }
  if (e != hipSuccess) {
    b.p = nullptr;
    // (the failed retry leaves its error behind in the runtime: a caller that falls back to a smaller size must not have its
    //  next launch check report this one)
    if (e == hipErrorOutOfMemory) (void)hipGetLastError();
    BCE_HIP_TRY(c, e);
  }
  c->alloc_s += now_s() - t0; c->alloc_bytes += bytes; c->alloc_calls++;
  if (now_s() - t0 > 0.02 && getenv("BCE_ALLOC_TRACE")) fprintf(stderr, "alloc: hipMalloc of %.1f MB took %.3f s\n", bytes / 1e6, now_s() - t0);
  b.cap = bytes;
  return BCE_HIP_OK;
}
// pinned host memory of the context (timed like the device allocations)
inline int pin_alloc(bce_hip_ctx *c, void **p, size_t bytes) {
  const double t0 = now_s();
  BCE_HIP_TRY(c, hipHostMalloc(p, bytes, hipHostMallocDefault));
  c->pin_s += now_s() - t0; c->pin_bytes += bytes; c->pin_calls++;
  return BCE_HIP_OK;
}
inline void release(DevBuf &b) {
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr; b.cap = 0;
}

// A few bytes from the device, now: through pinned memory of the context's own (a copy into pageable memory -- a stack
// variable -- goes through the runtime's staging buffers, which all host threads and contexts share).
inline int read_back(bce_hip_ctx *c, void *dst, const void *dev_src, size_t bytes) {
  if (bytes > 4096) return BCE_HIP_E_ARG;
  if (!c->h_small) BCE_TRY(pin_alloc(c, &c->h_small, 4096));
  BCE_HIP_TRY(c, hipMemcpyAsync(c->h_small, dev_src, bytes, hipMemcpyDeviceToHost, c->stream));
  BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
  memcpy(dst, c->h_small, bytes);
  return BCE_HIP_OK;
}

// C ABI boundary: no C++ exception may leave an entry point (a host allocation that fails in a std::vector, a thread that
// cannot be started): the heavy entry points run their body through this.
template <class F>
inline int bce_guarded(bce_hip_ctx *c, F &&body) {
  try { return body(); }
  catch (const std::bad_alloc &) { if (c) snprintf(c->err, sizeof c->err, "host allocation failed"); return BCE_HIP_E_NOMEM; }
  catch (const std::exception &e) { if (c) snprintf(c->err, sizeof c->err, "%s", e.what()); return BCE_HIP_E_INTERNAL; }
  catch (...) { if (c) snprintf(c->err, sizeof c->err, "unknown exception"); return BCE_HIP_E_INTERNAL; }
}

// The phase of an entry point (bce_hip_ctx::phase) for as long as it runs: every way out of it, error returns included, leaves
// phase 0 behind (a phase left standing would make a later ctx_trim give back buffers that are in use).
struct PhaseScope {
  PhaseScope(bce_hip_ctx *c, int phase) : c_(c) { c_->phase = phase; }
  ~PhaseScope() { c_->phase = 0; }
  void set(int phase) { c_->phase = phase; }     // an entry point that runs several phases in turn
  PhaseScope(const PhaseScope &) = delete;
  PhaseScope &operator=(const PhaseScope &) = delete;
 private:
  bce_hip_ctx *c_;
};

// roctx ranges around the kernel families (the reference's M_TIME stage lines, bce.cpp:886-891,974-979,1159-1164, as
// profiler markers: rocprofv3 --marker-trace shows K1 / K2 / K3 batches / K4 flushes on the host timeline).  The marker
// library is looked up at run time -- librocprofiler-sdk-roctx.so, else libroctx64.so -- and absent = no-op.
struct RoctxRange {
  explicit RoctxRange(const char *name);
  ~RoctxRange();
  RoctxRange(const RoctxRange &) = delete;
  RoctxRange &operator=(const RoctxRange &) = delete;
 private:
  bool on_;
};

constexpr uint32_t K3_TAIL_CAP = 1024;        // nodes the tail kernel holds in LDS (all 8 planes together)
constexpr uint32_t K3_SMALL_MAXTILES = 2048;  // tile table of the one-launch round kernel
#ifndef K3_SMALL_NODES_VALUE
#define K3_SMALL_NODES_VALUE 2000000u   // (1/2 M: 19.8 ms of K3 on the natural corpus, 1 M: 19.7, 1.5 M: 19.4, 2 M: 19.3; its tile table holds 2048.
                                        //  With a table of 4096: 3 M 19.5 vs 19.7 in the same run, 4 M 20.5; text 13.0 / 13.1 vs 12.9)
#endif
constexpr uint32_t K3_SMALL_NODES = K3_SMALL_NODES_VALUE;   // rounds up to this many nodes use it
constexpr uint32_t K3_TAIL_ENTER = 512;       // the host switches to the tail kernel at or below this many nodes
constexpr uint32_t K3_TAIL_MAXROUNDS = 65536; // rounds per tail launch (bounded by its run table)

inline uint32_t ceil_log2(uint32_t v) { uint32_t b = 0; while ((1ull << b) < v) ++b; return b; }

// ---- stage implementations (one .hip file each) ----
int k1_bwt(bce_hip_ctx *c);                         // k1_bwt.hip
// K1 in two halves, where k1_two_halves() says so (two bytes or more, below K1_PART_MIN elements): k1_first_sort orders the rotations by their first
// *h_symbols bytes, k1_provisional_bwt queues the BWT of that order into c->bwt, k1_finish is the rest of the sort and
// k1_final_bwt the BWT of the finished order (have_bwt: c->bwt holds it already) and offset_.  k1_bwt is all of it in one call.
// want_by_bits (or null): the depth the caller wants from the first sort, in symbols, indexed by the alphabet's width in bits
// (0: as many symbols as the key holds, what k1_bwt takes); the key carries the preceding byte where it has room for it
// (c->k1_carry).  BCE_K1_KEYBITS overrides the depth, BCE_HIP_CARRY_BYTE=0 the carry.
bool k1_two_halves(const bce_hip_ctx *c);
int k1_first_sort(bce_hip_ctx *c, uint32_t *h_symbols, const uint8_t *want_by_bits);
int k1_provisional_bwt(bce_hip_ctx *c);
int k1_finish(bce_hip_ctx *c);
int k1_final_bwt(bce_hip_ctx *c, bool have_bwt);
int k1_divbwt(bce_hip_ctx *c, const uint8_t *T_host, uint8_t *U_host, uint32_t n, uint32_t *pidx);   // the libdivsufsort seam
// The suffix array of n bytes (host memory, or device memory of the context's device) and, unless d_isa is null, its inverse,
// into device memory: k1_divbwt's sort, then kd_sufsort.hip's gather.  Complete on return.
int k1_suffix_array(bce_hip_ctx *c, const uint8_t *T_src, bool src_on_device, uint32_t n, uint32_t *d_sa, uint32_t *d_isa);
int kd_inverse_bw_transform(bce_hip_ctx *c, const uint8_t *T_host, uint8_t *U_host, uint32_t n, uint32_t idx);   // kd_backend.hip
// kd_backend.hip, test hooks: the decoder's planes() and inverse_bwt() stages on arrays of the caller's in device memory
int kd_planes_from_ranks(bce_hip_ctx *c, const uint32_t *d_R, uint32_t n, uint8_t *d_bwt, uint32_t *d_words, uint32_t *d_rankw);
int kd_unbwt(bce_hip_ctx *c, const uint8_t *d_bwt, uint32_t n, uint32_t offset, uint8_t *d_out, uint64_t *cycle, uint32_t *walkers);
int kd_compare(bce_hip_ctx *c, const uint8_t *a, const uint8_t *b, uint64_t m, uint64_t *first_diff);   // kd_compare.hip: first differing byte of two device buffers
int kd_crc32(bce_hip_ctx *c, const uint8_t *d, uint64_t n, uint32_t *crc);   // kd_crc32.hip: CRC-32 (zlib's) of a device buffer
// kd_count.hip: d_out[p] = occurrences of d_pat[d_off[p], d_off[p + 1]) in the circular text of the context's planes (device arrays)
int kd_count(bce_hip_ctx *c, const uint8_t *d_pat, const uint64_t *d_off, uint32_t npat, uint64_t *d_out);
// kd_locate.hip: the positions of the same occurrences, CSR.  _size: d_hits[npat + 1], their total and the batch's cyclic rows;
// _fill, straight after it: d_pos[total].  sa: K1's suffix array, null for n == 1.
int kd_locate_size(bce_hip_ctx *c, const uint32_t *sa, const uint8_t *d_pat, const uint64_t *d_off, uint32_t npat, bool linear,
                   uint64_t *d_hits, uint64_t *rows, uint64_t *total);
int kd_locate_fill(bce_hip_ctx *c, const uint32_t *sa, const uint64_t *d_off, uint32_t npat, bool linear, uint64_t rows, uint64_t total,
                   uint32_t *d_pos);
int locate_scan(bce_hip_ctx *c, const uint32_t *cnt, const uint32_t *drop, uint32_t npat, uint64_t *start, uint64_t *total);   // exclusive u64 scan of cnt - drop
// kd_near.hip: the same two questions within k <= BCE_HIP_NEAR_MAX_K mismatches (near_step.h).  Counts: d_out[npat * (k + 1)].  The
// locate's halves as kd_locate's, with the distance of every position beside it.
int kd_near_count(bce_hip_ctx *c, const uint8_t *d_pat, const uint64_t *d_off, uint32_t npat, uint32_t k, uint64_t *d_out);
int kd_near_size(bce_hip_ctx *c, const uint32_t *sa, const uint8_t *d_pat, const uint64_t *d_off, uint32_t npat, uint32_t k, bool linear,
                 uint64_t *d_hits, uint64_t *rows, uint64_t *total);
int kd_near_fill(bce_hip_ctx *c, const uint32_t *sa, const uint8_t *d_pat, const uint64_t *d_off, uint32_t npat, uint32_t k, bool linear,
                 uint64_t rows, uint64_t total, uint32_t *d_pos, uint8_t *d_dist);
// kd_edit.hip: the same two questions within k <= BCE_HIP_EDIT_MAX_K edits (edit_step.h), both reduced from candidates through the
// suffix array.  Counts: d_out[npat * (k + 1)], queued.  _size: the whole search, d_hits[npat + 1] and their total, and the sorted
// candidates (pos, tag) that _fill, straight after it, writes the heads of: d_pos, d_len, d_dist[total].
int kd_edit_count(bce_hip_ctx *c, const uint32_t *sa, const uint8_t *d_pat, const uint64_t *d_off, uint32_t npat, uint32_t k, bool linear,
                  uint64_t *d_out);
int kd_edit_size(bce_hip_ctx *c, const uint32_t *sa, const uint8_t *d_pat, const uint64_t *d_off, uint32_t npat, uint32_t k, bool linear,
                 uint64_t *d_hits, uint64_t *total, const uint32_t **pos, const uint32_t **tag);
int kd_edit_fill(bce_hip_ctx *c, const uint64_t *d_off, uint32_t npat, uint32_t k, const uint64_t *d_hits, uint64_t total, const uint32_t *pos,
                 const uint32_t *tag, uint32_t *d_pos, uint16_t *d_len, uint8_t *d_dist);
// kd_classes.hip: the same two questions for patterns of byte classes (class_step.h), under a budget of max_nodes search nodes per
// pattern.  d_masks: 8 words per class, d_off counts classes.  d_status[npat]: 0 or BCE_HIP_CLASS_OVER; d_work (may be null): the nodes.
int kd_class_count(bce_hip_ctx *c, const uint32_t *d_masks, const uint64_t *d_off, uint32_t npat, uint32_t max_nodes, uint64_t *d_counts,
                   uint64_t *d_work, uint32_t *d_status);
int kd_class_size(bce_hip_ctx *c, const uint32_t *sa, const uint32_t *d_masks, const uint64_t *d_off, uint32_t npat, uint32_t max_nodes, bool linear,
                  uint64_t *d_hits, uint32_t *d_status, uint64_t *rows, uint64_t *total);
int kd_class_fill(bce_hip_ctx *c, const uint32_t *sa, const uint32_t *d_masks, const uint64_t *d_off, uint32_t npat, uint32_t max_nodes, bool linear,
                  uint64_t rows, uint64_t total, const uint32_t *d_status, uint32_t *d_pos);
// kd_match.hip: d_len[i] (and d_pos[i], unless null) of the longest string that ends at d_query[i] and occurs in the text, at most
// max_len bytes; queued, the caller waits.  kd_coverage: the bytes of the query inside matches of min_len or more, from such lengths.
int kd_match(bce_hip_ctx *c, const uint32_t *sa, const uint8_t *d_query, uint32_t q, uint32_t max_len, bool linear, uint32_t *d_len,
             uint32_t *d_pos);
int kd_coverage(bce_hip_ctx *c, const uint32_t *d_len, uint32_t q, uint32_t min_len, uint64_t *covered);
// kd_lcp.hip: the LCP array of the sorted rotations of the circular text, capped at max_len (queued, the caller waits); the records
// of nk <= 64 values of k and the longest repeat, reduced from such an array of n words (both wait: the result's way back)
int kd_lcp(bce_hip_ctx *c, const uint32_t *sa, uint32_t max_len, uint32_t *d_lcp);
int kd_kgrams(bce_hip_ctx *c, const uint32_t *sa, const uint32_t *d_lcp, uint32_t n, const uint32_t *ks, uint32_t nk, bce_hip_kgram *out);
int kd_longest_repeat(bce_hip_ctx *c, const uint32_t *sa, const uint32_t *d_lcp, uint32_t n, uint32_t res[3]);
// the first min(limit, distinct) classes of k by size descending, first row ascending, into device memory; complete on return
int kd_top_kgrams(bce_hip_ctx *c, const uint32_t *sa, const uint32_t *d_lcp, uint32_t n, const uint8_t *text, uint32_t k, uint32_t limit,
                  bce_hip_top_kgram *d_out, uint8_t *d_bytes, uint32_t *found, uint64_t *distinct, uint64_t size_hist[32]);
// kd_parse.hip: the query as copies out of the text plus literal bytes, from its lengths and positions; and back.  Both wait.
int kd_parse(bce_hip_ctx *c, const uint32_t *d_len, const uint32_t *d_pos, const uint8_t *d_query, uint32_t q, uint32_t min_len, bool sizing,
             uint32_t *d_ops, uint64_t ops_cap, uint8_t *d_lits, uint64_t lits_cap, bce_hip_parse_info *info);
int kd_patch(bce_hip_ctx *c, const uint32_t *d_ops, uint32_t nops, const uint8_t *d_lits, uint64_t nlits, bool sizing, uint8_t *d_out,
             uint64_t cap, uint64_t *out_len);
// kd_self.hip: all nearest smaller values of n words; the longest previous factor of every text position (at n - 1 - i: mirror);
// the mirrors of lengths, sources and text in slf_rlen / slf_rsrc / slf_rtext; kd_parse's chain over those, turned round.  The
// first three are queued and the caller waits; the last is complete on return.
int kd_nsv(bce_hip_ctx *c, const uint32_t *d_vals, uint32_t n, uint32_t *d_psv, uint32_t *d_nsv);
constexpr uint32_t NSV_TREE_BLOCK = 2048;           // rows per block tree
// the blocks' trees and the top tree over vals[0, n), n >= 1, into slf_tree / slf_top, *NB_out = the top tree's leaves; queued
int nsv_trees(bce_hip_ctx *c, const uint32_t *vals, uint32_t n, uint32_t *NB_out);
// kd_maxrep.hip: the maximal repeats of n >= 2 rows from the capped LCP array in rep_lcp (32-byte aligned, d_lcp), heaviest first
// (maxrep_step.h).  bw: null (the preceding bytes come from sa and text) or n bytes in their place; d_bytes: null, or room for
// limit * bytes_per bytes, then `text` is read.  info->found entries are written to d_out; complete on return.
int kd_maxrep(bce_hip_ctx *c, const uint32_t *sa, const uint32_t *d_lcp, uint32_t n, const uint8_t *text, const uint8_t *bw, uint32_t min_len,
              uint32_t max_len, uint32_t order, uint32_t limit, bce_hip_maxrep *d_out, uint8_t *d_bytes, uint32_t bytes_per, bce_hip_maxrep_info *info);
int kd_lpf(bce_hip_ctx *c, const uint32_t *sa, uint32_t max_len, bool mirror, uint32_t *d_lpf, uint32_t *d_src);
int kd_self_mirror(bce_hip_ctx *c, const uint32_t *d_lpf, const uint32_t *d_src, const uint8_t *d_text, uint32_t n);
int kd_self_parse(bce_hip_ctx *c, uint32_t n, uint32_t min_len, bool with_src, bool sizing, uint32_t *d_ops, uint64_t ops_cap, uint8_t *d_lits,
                  uint64_t lits_cap, bce_hip_parse_info *info);
// kd_sufsort.hip: rows 1 .. n of K1's order of T$ and the rank array as suffix array and inverse (queued, the caller waits); the
// verdict on n words as a suffix array of n bytes, both in device memory (complete on return)
int kd_sa_gather(bce_hip_ctx *c, const uint32_t *sa, const uint32_t *rank, uint32_t n, uint32_t *d_sa, uint32_t *d_isa);
int kd_sufcheck(bce_hip_ctx *c, const uint8_t *d_text, const uint32_t *d_sa, uint32_t n, uint64_t *bad, uint32_t *reason);
int k2_build_planes(bce_hip_ctx *c);                // k2_planes.hip
int k2_get_plane_bits(bce_hip_ctx *c, int plane, uint8_t *out);
int k2_rank1(bce_hip_ctx *c, int plane, const uint32_t *idx, uint32_t count, uint32_t *out);
int k3_begin(bce_hip_ctx *c);                       // k3_enumerate.hip
int k3_rounds(bce_hip_ctx *c, uint32_t count, uint64_t nodes_hint);   // queue `count` rounds from c->round (no sync)
int k3_rounds_small(bce_hip_ctx *c, uint32_t count, uint64_t cur_nodes, bool growing);   // one launch per round, narrow rounds
int k3_round_masked(bce_hip_ctx *c, uint32_t mask, bool repeat);   // one round, three launches, symbols of the planes in `mask` only
int k3_clear_need_flush(bce_hip_ctx *c);
int k3_clear_small_bail(bce_hip_ctx *c);   // after a one-launch round bailed out: small_bail = 0, so that later launches run again
int k3_dfs_tail(bce_hip_ctx *c, const EnumCtl &ctl, uint32_t enter, bool *done);   // k3_dfs.hip: finish the enumeration depth-first
int k3_tail(bce_hip_ctx *c, uint32_t max_rounds = K3_TAIL_MAXROUNDS);   // queue the persistent narrow-round kernel from c->round (no sync)
int k3_fetch_tail_runs(bce_hip_ctx *c, uint32_t rounds);
int k3_sync_ctl(bce_hip_ctx *c, EnumCtl *out);      // copy the control block back (syncs the stream)
int k3_fetch_runs(bce_hip_ctx *c, uint32_t first_round, uint32_t count);  // append run-table rows to run_log
int k3_get_nodes(bce_hip_ctx *c, int plane, uint32_t *out, uint32_t cap, uint32_t *count);
int k3_reset_symbols(bce_hip_ctx *c);               // after a flush: sym_total = 0, need_flush = 0
int k3_grow_symbols(bce_hip_ctx *c, uint64_t cap);  // enlarge the (empty) symbol buffer, clear need_flush
int k4_prepare(bce_hip_ctx *c);                     // k4_model.hip: counters to zero, cfg upload
int k3_grow_lists(bce_hip_ctx *c, const EnumCtl &ctl);
uint64_t k3_symbol_capacity(const bce_hip_ctx *c, uint32_t n);   // records between two model flushes for an input of n bytes
void k4_prepin(bce_hip_ctx *c, uint32_t n);         // start pinning the flush slots' host staging for an input of n bytes (threads)
void k4_prepin_join(bce_hip_ctx *c, bool drop);     // wait for those threads (drop: free what they pinned and nobody adopted)
int k4_flush(bce_hip_ctx *c, uint64_t nsym, FlushSlot &slot);         // synchronous: outputs are in slot.h_out on return
// sort + replay + D2H into the slot, all queued: outputs are in slot.h_out once slot.ev_copy has fired.  copy_out = false
// (estimate mode): the records stay in `sout`, the slot needs no host staging and only lends its events.
int k4_flush_async(bce_hip_ctx *c, uint64_t nsym, FlushSlot &slot, bool copy_out = true);
int k4_long_runs(bce_hip_ctx *c, uint64_t nsym, uint32_t *count);    // test hook: long runs queued by the flush of nsym records that has just completed
int k4_cost_begin(bce_hip_ctx *c);                  // k4_cost.hip: the context's sums to zero
int k4_cost_async(bce_hip_ctx *c, uint64_t nsym, FlushSlot &slot);   // behind k4_flush_async(.., false): add the flush's code lengths, per plane
int k4_cost_end(bce_hip_ctx *c, uint64_t acc[16]);  // wait and read them: [0..7] Q24 cost sums, [8..15] record counts

// radix sort (radix_sort.hip): stable LSD sort of (key,val) u32 pairs on key bits [first_bit, first_bit+bits).
// Result is left in key[res]/val[res]; returns res (0 or 1) through *res.  first_bit + bits > 32: BCE_HIP_E_ARG.
int radix_sort_pairs(bce_hip_ctx *c, uint32_t *key[2], uint32_t *val[2], uint32_t n, uint32_t first_bit, uint32_t bits, int *res,
                     uint32_t max_digit_bits = 8);
int radix_sort_pairs_on(bce_hip_ctx *c, hipStream_t stream, DevBuf &hist, uint32_t *key[2], uint32_t *val[2], uint32_t n,
                        uint32_t first_bit, uint32_t bits, int *res, uint32_t max_digit_bits = 8);
// the same with 64-bit keys in two u32 arrays (hi:lo) on key bits [0, bits), bits <= 64 (K1's first sort)
int radix_sort_wide(bce_hip_ctx *c, uint32_t *lo[2], uint32_t *hi[2], uint32_t *val[2], uint32_t n, uint32_t first_bit, uint32_t bits, int *res,
                    uint32_t max_digit_bits = 10);
bool k4_in_flight(bce_hip_ctx *c);                  // a model flush may still be running beside the main stream

}  // namespace bce
