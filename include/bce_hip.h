/*
 * bce_hip.h -- C ABI of libbcehip.so, the MI355X (gfx950) implementation of the `bce -c` hot path.
 *
 * The reference (akamiru/bce, /root/reference/bce.cpp) exposes no FFI; its seams are C++ template
 * policies inside one translation unit plus the libdivsufsort C ABI.  Each entry point below names
 * the reference interface it replaces (file:line).  All functions return 0 on success and a negative
 * bce_hip_status on failure (the reference's convention is status ints + printf, no exceptions:
 * CMakeLists.txt:25).  The context owns every device buffer; callers own every host buffer they
 * pass.  A context is used from one host thread at a time.
 */
#ifndef BCE_HIP_H
#define BCE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bce_hip_ctx bce_hip_ctx;

enum bce_hip_status {
  BCE_HIP_OK = 0,
  BCE_HIP_E_ARG = -1,       /* bad argument (null pointer, n == 0, n >= 2^31, wrong config size) */
  BCE_HIP_E_DEVICE = -2,    /* HIP runtime error (no device, launch failure, ...) */
  BCE_HIP_E_NOMEM = -3,     /* device or host allocation failed */
  BCE_HIP_E_STATE = -4,     /* stage called out of order */
  BCE_HIP_E_OVERFLOW = -5,  /* output buffer too small / internal capacity exceeded */
  BCE_HIP_E_INTERNAL = -6   /* device-side consistency check failed */
};

#define BCE_HIP_CONFIG_BYTES 288u /* (31+1)*9, bce.cpp:629 */

/* ---- lifetime ---------------------------------------------------------------------------------- */
int bce_hip_create(bce_hip_ctx **out, int device);
/* The same for a one-shot caller that knows the size of the input it is about to compress (`bce -c`: the file's size, main()
 * bce.cpp:1403-1427): host-side preparation that depends on it -- the pinned staging of the model flushes, 8 bytes per
 * symbol record of a flush in three slots: 3 x 8 MB from 128 KB of input, 3 x 128 MB from 2 MB up -- runs on threads of
 * its own beside the HIP runtime's initialisation instead of inside the first compression.  A hint only: any input may
 * follow; 0 = unknown (= bce_hip_create). */
int bce_hip_create_sized(bce_hip_ctx **out, int device, uint64_t expected_input_bytes);
void bce_hip_destroy(bce_hip_ctx *ctx);
const char *bce_hip_strerror(int status);
/* last HIP error string seen by this context (for diagnostics) */
const char *bce_hip_last_error(const bce_hip_ctx *ctx);

/* ---- configuration ----------------------------------------------------------------------------- */
/* AdaptiveCoder<31>::load_config (bce.cpp:626-641): 9 rows x 32 context-bit counts.  NULL restores
 * the built-in defaults (bce.cpp:713-724). */
int bce_hip_set_config(bce_hip_ctx *ctx, const uint8_t *config288);
/* Several contexts on ONE device (a stream of files or blocks, `bce -cN` with more blocks than GPUs): a compression is a
 * GPU phase followed by a host phase in which the eight coder threads finish the last batches, so contexts driven by
 * one host thread each overlap one's coding -- and one's rotation sort -- with the other's enumeration.  Gated contexts
 * of a device take turns for the ENUMERATION (its single-launch rounds must not run beside another context's):
 * bce_hip_encode / bce_hip_scan take the device's gate, give it back when the last model flush is queued or when they
 * fail, and lend it to the next context while they wait for their own coder threads and -- since round 4 -- behind every model
 * flush they queue (the model's kernels wait for nothing; the gate comes back before the next round is queued);
 * bce_hip_destroy and this call (with either value) give it back too.  Every context is gated by default (an uncontended gate costs nothing); contexts of
 * other PROCESSES on the same device are kept apart by an advisory file lock keyed by the device's PCI address
 * (/dev/shm/bce_hip_gate_<bdf>; BCE_HIP_NO_FILE_GATE=1 switches that part off).  on = 0 opts a context out: only for
 * a context that is alone on its device. */
int bce_hip_set_gated(bce_hip_ctx *ctx, int on);
/* capacity (in symbol records) of the device symbol buffer between model flushes; 0 = automatic */
int bce_hip_set_symbol_capacity(bce_hip_ctx *ctx, uint64_t records);

/* Progress of BCE::code (the reference prints "Coded: %u.%02u %%\r" from it, bce.cpp:1354-1358): called from the calling
 * thread with the nodes visited so far and the total (8n) whenever the host looks at the enumeration's state, during
 * bce_hip_encode / _compress / _scan / _decompress_device.  NULL switches it off (default). */
typedef void (*bce_hip_progress_fn)(uint64_t nodes_done, uint64_t nodes_total, void *user);
int bce_hip_set_progress(bce_hip_ctx *ctx, bce_hip_progress_fn fn, void *user);

/* test knobs for the enumeration's alternative code paths (all 0 by default): 0 = nodes a depth-first walker
 * classifies per pass, 1 = disable the depth-first tail, 2 = disable the persistent LDS tail kernel, 3 = disable chain skipping, 4 = disable the one-launch kernel for narrow rounds, 6 = three launches per wide round (separate scan kernel) instead of two, 7 = disable the workgroup-local rounds before the depth-first tail,
 * 8 = live nodes below which the walkers take over from the workgroup-local rounds (default 16 384; the tail itself starts at 1 M live nodes with the local rounds, at 65 536 without them: BCE_HIP_DFS_ENTER), 9 = rounds a workgroup runs per pass before it hands on (default 192),
 * 10 = round from which the tail may start although the node count still grows (exercises the spill path),
 * 11 = model flushes (K4) on a stream of their own beside the next K3 rounds, double-buffered symbol records (also BCE_HIP_OVERLAP=1),
 * 12 = d: the node lists start with n / d + 4096 nodes instead of n / 8 + 4096 (also BCE_HIP_CAPP_DIV=d; large d: the lists grow many times).
 * 13 = B: the GPU-assisted decoder's query budget, the nodes one pass of a round may hold (default 2^30, 0 = default, values below
 *      4096 count as 4096): a round with more nodes runs plane group by plane group (bce_hip_stats.dec_split_rounds).
 * 14 = m: device allocations of this context that fail for real -- hipMalloc is asked for hipMemGetInfo's total + 1 GiB, so the
 *      runtime's own out-of-memory error is what the code sees and what stays set until it is read, as on a full device.
 *      1 = both attempts at a node list's first-choice size (encoder k3_grow_lists, decoder grow_lists: their fallback sizes
 *      succeed), 2 = every attempt of a node list's growth (BCE_HIP_E_NOMEM, "no device memory for ... node list(s) of ..."),
 *      3 = the first attempt of every allocation (the retry after the other phases' buffers have gone back succeeds); 0 = off.
 * The archive never depends on them. */
int bce_hip_debug_set(bce_hip_ctx *ctx, int knob, uint32_t value);

/* ---- stage 0: input ---------------------------------------------------------------------------- */
/* File::File (bce.cpp:842-856): take the n input bytes.  _host copies host->HBM, _device copies
 * HBM->HBM from a device pointer of the same GPU (input already resident). 1 <= n < 2^31.
 * Capacity: device memory is ~45 n bytes for the suffix sort and planes plus the enumeration's node lists: 16 lists (8 planes x
 * the two parities of a round) that start with n/8 nodes each (text fills 0.02-0.03 n, random bytes 0.15-0.3 n).  A round whose
 * children do not fit is not run: the lists it would write -- the other parity's, empty at that moment -- are replaced by larger
 * ones (bce_hip_stats.list_grows; no copy, never old and new side by side), up to the worst case of n/2 + 2 nodes, and when the
 * device runs out of memory the buffers of the stages that are not running (the suffix sort's scratch) go back first.  Every
 * valid input -- any 1 <= n < 2^31, as the reference (bce.cpp:173,374,901) -- fits an otherwise idle 288 GB MI355X: the worst
 * case is 72 n bytes of lists beside 13 n bytes that stay.  A round that emits more symbols than one model flush takes (2^31
 * records) is run plane group by plane group (bce_hip_stats.split_rounds).  The GPU-assisted DECODER, bce_hip_decompress_device,
 * holds 32 n bytes of boundary ranks beside 16 node lists of their own per (parity, plane) -- at most 72 n bytes together, each
 * list grown in place when a round's children do not fit (bce_hip_stats.dec_list_grows) -- and per-round query buffers bounded by
 * a budget of 2^30 queries (a wider round runs plane group by plane group: dec_split_rounds); after the rounds the lists and query
 * buffers go back before the planes and the inverse BWT allocate, where free memory would be short.  Largest archive decoded: 2^31 - 2 random bytes (2 166 438 056 B). */
int bce_hip_load_host(bce_hip_ctx *ctx, const uint8_t *in, uint32_t n);
int bce_hip_load_device(bce_hip_ctx *ctx, const void *d_in, uint32_t n);

/* ---- stage 1 (K1): rotation + BWT --------------------------------------------------------------- */
/* File::rotate + File::bwt (bce.cpp:858-910), i.e. the libdivsufsort call
 *   saidx_t divbwt(const sauchar_t *T, sauchar_t *U, saidx_t *A, saidx_t n)   (bce.cpp:901)
 * plus the two std::rotate fix-ups: sorts all cyclic rotations on the GPU, leaves the n-byte BWT in
 * HBM and returns offset_ (index of the first minimal rotation, bce.cpp:893). */
int bce_hip_bwt(bce_hip_ctx *ctx, uint32_t *offset);
/* Test hook: inject a BWT computed elsewhere instead of running K1. */
int bce_hip_set_bwt(bce_hip_ctx *ctx, const uint8_t *bwt, uint32_t n, uint32_t offset);
/* Copy the BWT bytes back (n bytes). */
int bce_hip_get_bwt(bce_hip_ctx *ctx, uint8_t *bwt_out);

/* The libdivsufsort seam itself (bce.cpp:901, :1091): the two functions of that library's C ABI which the reference calls,
 * with their argument meaning, on a context (include/divsufsort_hip.h + libdivsufsort_hip.so wrap them under their
 * original names and signatures, so that an unmodified bce.cpp links against them).  Host buffers; in == out allowed.
 * divbwt: BWT of in[0, n) with an implicit smallest sentinel, *primary = 1-based row of suffix 0.  The context's
 * compression state is dropped by either call. */
int bce_hip_divbwt(bce_hip_ctx *ctx, const uint8_t *in, uint8_t *out, uint32_t n, uint32_t *primary);
int bce_hip_inverse_bwt(bce_hip_ctx *ctx, const uint8_t *in, uint8_t *out, uint32_t n, uint32_t primary);

/* ---- stage 2 (K2): wavelet-matrix bit planes + rank directory ----------------------------------- */
/* RankFile ctor body + Rank::build (bce.cpp:944-970, 138-145).  zeros[j] = rank0_j(n). */
int bce_hip_build_planes(bce_hip_ctx *ctx, uint32_t zeros[8]);
/* Test hook: plane j, positions [0,n) -> one byte (0/1) each, as Rank::bit (bce.cpp:196-198). */
int bce_hip_get_plane_bits(bce_hip_ctx *ctx, int plane, uint8_t *bits_out);
/* Test hook: rank1_j(index) for an array of query positions, as Rank::get<1> (bce.cpp:147-151). */
int bce_hip_rank1(bce_hip_ctx *ctx, int plane, const uint32_t *idx, uint32_t count, uint32_t *out);

/* ---- stage 3+4 (K3, K4) + host coder: BCE::encode ------------------------------------------------ */
/* BCE::encode (bce.cpp:1117-1167): runs BCE::code mode 1 (bce.cpp:1236-1374) as per-round GPU
 * passes (K3), the AdaptiveCoder model half (bce.cpp:506-518,531-533,671-677) on the GPU (K4), the
 * range-coder half (bce.cpp:520-529,538-553,610-615,655-661) on 8 host threads, then frames the
 * archive (bce.cpp:1140-1157).  The archive is kept in the context until the next load. */
int bce_hip_encode(bce_hip_ctx *ctx);
/* size of / copy of the finished archive (native-endian u16 words, bce.cpp:1426) */
int bce_hip_archive_size(bce_hip_ctx *ctx, size_t *bytes);
int bce_hip_archive_copy(bce_hip_ctx *ctx, uint8_t *out, size_t cap);

/* ---- extension: ONE archive from several contexts / GPUs (SURVEY section 8e-2's aim) ------------------
 * The eight plane coders of BCE::encode (bce.cpp:1124-1150) are independent sequential streams; the archive is header +
 * the eight streams (:1152-1157).  A context codes only the planes of `mask` (bit p = plane p; default 0xFF; set before
 * bce_hip_encode, it stays until changed); after bce_hip_encode the finished stream of a plane it owns can be read, and
 * the stream of a plane another context owns can be put in its place -- the header is coded again from the new sizes --
 * so that bce_hip_archive_size / _copy give the archive `bce -c` writes.  Every context must have encoded the same input
 * with the same config.  Streams are native-endian u16 words. */
int bce_hip_set_plane_mask(bce_hip_ctx *ctx, uint32_t mask);
int bce_hip_plane_stream_size(bce_hip_ctx *ctx, int plane, size_t *words);
int bce_hip_plane_stream_copy(bce_hip_ctx *ctx, int plane, uint16_t *out, size_t cap_words);
int bce_hip_plane_stream_set(bce_hip_ctx *ctx, int plane, const uint16_t *words, size_t count);

/* ---- one-shot: main() -c branch minus file I/O (bce.cpp:1403-1427) -------------------------------- */
int bce_hip_compress(bce_hip_ctx *ctx, const uint8_t *in, uint32_t n, uint8_t *out, size_t cap, size_t *out_len);
/* same with the input already in HBM */
int bce_hip_compress_device(bce_hip_ctx *ctx, const void *d_in, uint32_t n, uint8_t *out, size_t cap, size_t *out_len);

/* ---- extension: the archive's size without coding it (k4_cost.hip) ---------------------------------------------------------
 * BCE::encode (bce.cpp:1117-1167) with the range coders left out: K3 and K4 run as for bce_hip_encode, and where the host coders
 * would take the model's (cum, freq, total) records (AdaptiveCoder::set's coder half, bce.cpp:520-529; the k > 31 escape's uniform
 * bits, :507-510) a kernel adds up what each step costs, log2(total / freq) bits, per plane, where the records lie.  Nothing is
 * copied to the host but 128 bytes at the end; no archive is made and none that the context holds is touched.
 * Preconditions: those of bce_hip_encode (after bce_hip_build_planes; the config in force is the one bce_hip_set_config set).
 * A later bce_hip_encode on the same context gives the archive it would have given without the estimate.  bce_hip_set_plane_mask
 * is not looked at -- the estimate's rounds record every plane's symbols -- and stays as it was: the estimate is of the whole archive.  Any of the three outputs may be NULL.
 *   plane_cost_q24[p]  bits, in unsigned Q24 fixed point (2^24 = one bit), of everything plane p's coder codes: the preamble of
 *                      its config row and C[p] (bce.cpp:682-691, :1128) and every step of its records.  Integer sums of
 *                      bce_hip_cost_q24: independent of how rounds and flushes are cut, the same from run to run.
 *   plane_steps[p]     the adaptive coder's calls for plane p (coder_[p].set(...), bce.cpp:1302) = its model records; their sum
 *                      is bce_hip_stats.symbols.  (A record with a k > 31 escape costs its uniform bits too, but counts once.)
 *   *archive_bytes     2 x (1 + header words + the eight streams' words): a stream is the whole 16-bit words of its sum
 *                      (shift_out, bce.cpp:655-661) plus the one word flush() adds (:610-615), which carries the rest; the
 *                      header coder main(-1) (bce.cpp:1141-1150) is run on those sizes.  Measured against the real archive:
 *                      DESIGN.md section 4.7.
 * bce_hip_stats afterwards: as after bce_hip_encode, with t_coder = t_coder_busy = 0; t_model is K4 plus the cost kernel. */
int bce_hip_estimate(bce_hip_ctx *ctx, uint64_t plane_cost_q24[8], uint64_t plane_steps[8], size_t *archive_bytes);
/* load + BWT + planes + estimate in one call: main() -c branch (bce.cpp:1403-1427) up to the coders, like bce_hip_compress /
 * bce_hip_compress_device.  A null ctx or input, n == 0 or n >= 2^31: BCE_HIP_E_ARG before any device call. */
int bce_hip_estimate_host(bce_hip_ctx *ctx, const uint8_t *in, uint32_t n, uint64_t plane_cost_q24[8], uint64_t plane_steps[8],
                          size_t *archive_bytes);
int bce_hip_estimate_device(bce_hip_ctx *ctx, const void *d_in, uint32_t n, uint64_t plane_cost_q24[8], uint64_t plane_steps[8],
                            size_t *archive_bytes);
/* The cost of one range-coder step encode(cum, freq, total) (bce.cpp:520-529): L(total) - L(freq), L = log2 in unsigned Q24,
 * integer arithmetic only (bce_amd/csrc/bce_cost.h: the function the kernel runs, compiled for the host).  1 <= freq <= total;
 * anything else gives 0.  Uses no GPU. */
uint32_t bce_hip_cost_q24(uint32_t freq, uint32_t total);

/* ---- stepping interface for parity tests (BCE::code one round at a time) --------------------------- */
/* begin: sets up the roots (bce.cpp:1237-1240).  round: runs one round over all 8 planes and
 * reports how many nodes the NEXT round holds.  nodes: copies plane p's current node list as
 * (s absolute, x0, x1) triples, sorted by s (j=0 list then j=1 list, bce.cpp:1256-1264). */
int bce_hip_enum_begin(bce_hip_ctx *ctx);
int bce_hip_enum_nodes(bce_hip_ctx *ctx, int plane, uint32_t *triples_out, uint32_t cap_nodes, uint32_t *count);
int bce_hip_enum_round(bce_hip_ctx *ctx, uint64_t *next_nodes);
/* symbol records emitted so far and not yet flushed, in (round, plane, s) order.  Each record:
 * out[6*i+0..5] = plane, s, k, nesc, escbits, slot  (s,k after the k>31 escape, bce.cpp:507-510) */
int bce_hip_enum_symbols(bce_hip_ctx *ctx, uint32_t *out, uint64_t cap_records, uint64_t *count);
/* run K4 on the symbols emitted so far: out[3*i+0..2] = cum, freq, total per record (same order) */
int bce_hip_enum_model(bce_hip_ctx *ctx, uint32_t *out, uint64_t cap_records, uint64_t *count);

/* Test hook: K4 (k4_model.hip) alone, on records of the caller's choosing instead of those K3 happens to emit.
 * begin: the model of the config in force (bce_hip_set_config) with all counters zero; needs no loaded input and ends a stepped
 * enumeration of the context.  flush: `count` symbol records in stream order -- key_words[i] / esc_words[i] as bce_core.h's
 * pack_symbol lays them out: key [4:0] sym, [9:5] k, [25:10] slot, [28:26] plane; esc [26:0] escape bits, [31:27] nesc -- go where
 * K3 would have left them and through the flush bce_hip_enum_model runs; out_records[i] = the raw 64-bit model record of record i
 * (pack_model_out: cum, freq - 1, total, escape bits with their sentinel), *long_runs (may be NULL) = the runs of 256 and more
 * records of one slot that this flush handed to the long-run kernels.  The counters stay for the next flush; count == 0 does
 * nothing and succeeds.  Every record is checked on the host before any device work: plane < 8, 2 <= k <= 31, sym < k, the slot
 * inside [ctxoff[k], ctxoff[k] + 4^bits[k]) of its plane's config row, nesc <= 27, nesc > 0 only with k >= 16, no escape bit at
 * or above nesc; one that fails any of them: BCE_HIP_E_ARG, nothing uploaded, the counters untouched, the context usable.
 * Without a begin: BCE_HIP_E_STATE. */
int bce_hip_model_begin(bce_hip_ctx *ctx);
int bce_hip_model_flush(bce_hip_ctx *ctx, const uint32_t *key_words, const uint32_t *esc_words, uint64_t count,
                        uint64_t *out_records, uint32_t *long_runs);

/* ---- config scan (SURVEY section 8f "next #2") ---------------------------------------------------------------- */
/* main() -s branch (bce.cpp:1384-1402): BCE<ScanCoder<31>, noop>::encode + ScanCoder::save_config
 * (bce.cpp:726-834).  Call after bce_hip_build_planes: the enumeration runs on the GPU, the eight ScanCoders and
 * their cost optimisation on the host.  config288 = the .bcc file content; result_bytes[9] (optional) = the values
 * of the nine "Result size: %.1f B" lines (bce.cpp:799). */
int bce_hip_scan(bce_hip_ctx *ctx, uint8_t config288[BCE_HIP_CONFIG_BYTES], double result_bytes[9]);
/* Test hook (tests/test_gpu_scan_routes.py): bce_hip_scan with the ScanCoders left out -- the same body (stage check, gate, scan
 * mode, enumeration, the per-flush copy and its spans) hands every flush's words to a plain sink instead.  Each word is one
 * symbol as bce_core.h's scan_pack lays it out: [4:0] sym, [9:5] k (2..31), [17:10] (c1 << 8) / cs, [25:18] (c2 << 8) / cs,
 * [30:26] k > 31 escapes.  Stream p = plane p's spans of every flush, in order: what ScanCoder p is fed.  counts[p] = the words of
 * stream p; out receives the streams of planes 0..7 back to back.  Their sum above cap_words: BCE_HIP_E_OVERFLOW with counts
 * filled and out untouched (out may be NULL with cap_words == 0: a sizing call, which runs the enumeration all the same).
 * bce_hip_stats afterwards reads as after bce_hip_scan.  Before bce_hip_build_planes: BCE_HIP_E_STATE; then a null counts, or a
 * null out with cap_words > 0: BCE_HIP_E_ARG. */
int bce_hip_scan_records(bce_hip_ctx *ctx, uint32_t *out, uint64_t cap_words, uint64_t counts[8]);

/* ---- decoder (SURVEY section 8f "next #1"): bce_hip_decompress = plain host C++ (`bce -ds`),
 *      bce_hip_decompress_device = the GPU-assisted decoder of kd_decode.hip (`bce -d`); same bytes.
 *      The GPU-assisted decoder has one body and three destinations for the text: the caller's host buffer
 *      (bce_hip_decompress_device), the caller's device memory (bce_hip_decompress_to_device: the mirror of
 *      bce_hip_compress_device, nothing of the text crosses to the host), or none -- compared on the device with the
 *      original (bce_hip_verify_device / _host, `bce -t`: the format carries no checksum, so "decode it and compare" is
 *      the integrity check there is -- for a plain archive; a version-2 container carries CRC-32s, see the CRC-32 section below).  The archive is a host pointer in all of them: the eight range decoders read it
 *      on host threads.  All work runs on the context's own stream and is complete when the call returns; device
 *      memory the caller passes in must be ready (its producer's stream synchronised) when the call is made. -------- */
/* BCE::decode + unbwt::bytewise + inverse BWT + rotate (bce.cpp:1169-1233, 1043-1102): archive -> original bytes.
 * out == NULL: only report the decoded size in *out_len.  Needs no context and no GPU. */
int bce_hip_decompress(const uint8_t *archive, size_t len, uint8_t *out, size_t cap, size_t *out_len);
/* Same result with the GPU doing everything but the eight sequential range decoders + adaptive models (kd_decode.hip):
 * node classification, children and boundary ranks per round on the device, the decoders' answers on 8 host threads,
 * then plane fill, unbwt::bytewise as wavelet-matrix access and the inverse BWT on the device.  Uses the context's
 * device, stream and scratch buffers; a compression in progress in the same context is dropped. */
int bce_hip_decompress_device(bce_hip_ctx *ctx, const uint8_t *archive, size_t len, uint8_t *out, size_t cap, size_t *out_len);
/* The same decode with the text left in DEVICE memory the caller owns (of the context's device; any alignment, e.g. a slice of a
 * tensor): the inverse BWT writes its bytes straight to d_out[0, n), never beyond, and the context allocates no text buffer of its
 * own.  d_out == NULL: only report the decoded size; cap < n: BCE_HIP_E_OVERFLOW, nothing written. */
int bce_hip_decompress_to_device(bce_hip_ctx *ctx, const uint8_t *archive, size_t len, void *d_out, size_t cap, size_t *out_len);
/* Decode into the context's own buffer and compare there with the n bytes of the original (_device: device memory of the context's
 * device, any alignment; _host: uploaded once into a scratch buffer of the context that is idle by then).  BCE_HIP_OK with
 * *first_diff = UINT64_MAX: the archive decodes to exactly these n bytes; = i: the smallest index at which the two differ; the
 * sizes differ and the common prefix agrees: min(n, decoded size).  An archive that does not parse or decode: the decoder's status,
 * as bce_hip_decompress_device, *first_diff untouched. */
int bce_hip_verify_device(bce_hip_ctx *ctx, const uint8_t *archive, size_t len, const void *d_original, size_t n, uint64_t *first_diff);
int bce_hip_verify_host(bce_hip_ctx *ctx, const uint8_t *archive, size_t len, const uint8_t *original, size_t n, uint64_t *first_diff);

/* ---- extension: CRC-32 of texts, on the host and on the device (the blocks of a version-2 BCEM container) --------------
 * A plain archive carries no checksum and must not: it is the reference's format.  The multi-block container is this project's
 * own; its version 2 (`bce -CN`, bce_amd/container.py) holds the CRC-32 of every block's text -- as zlib, gzip and PNG compute it:
 * reflected polynomial 0xEDB88320, init and final xor 0xFFFFFFFF -- so that an archive can be tested without the original. */
/* zlib's calling shape: `crc` of the bytes so far (0 to start) -> crc of those bytes followed by p[0, n).  Host code, no context,
 * no GPU. */
uint32_t bce_hip_crc32(uint32_t crc, const uint8_t *p, size_t n);
/* CRC-32 of A || B from the CRC-32s of A and of B and the length of B (any 64-bit length; the bytes are not needed): crc_a times
 * x^(8 len_b) mod P by square and multiply, plus crc_b.  Gives a whole file's CRC from its blocks'.  Host code, no GPU. */
uint32_t bce_hip_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);
/* CRC-32 of n bytes of device memory of the context's device (any alignment, any n -- 2^32 and more included), computed there
 * (kd_crc32.hip): one read of the bytes, one word comes back.  Stream rule of bce_hip_decompress_to_device: runs on the
 * context's stream, complete on return; the memory must be ready when the call is made.  n == 0: *crc = 0, d ignored.  A null
 * ctx or crc: BCE_HIP_E_ARG before any device call. */
int bce_hip_crc32_device(bce_hip_ctx *ctx, const void *d, size_t n, uint32_t *crc);
/* CRC-32 of the input the context holds, on the device.  Valid from bce_hip_load_host / _device on for as long as the context
 * keeps the input's bytes: through bce_hip_bwt, bce_hip_build_planes, bce_hip_encode / _scan and after them (the depth-first tail
 * of the enumeration reads the text, so no stage gives it back), until the next call that takes the buffer for something else --
 * a load, bce_hip_set_bwt, bce_hip_divbwt, bce_hip_inverse_bwt or any decode in this context.  Otherwise BCE_HIP_E_STATE. */
int bce_hip_input_crc32(bce_hip_ctx *ctx, uint32_t *crc);
/* The GPU-assisted decode with the text left in the context's own buffer and only its size and CRC-32 reported: no second buffer
 * is held and nothing of the text goes to the host (`bce -t archive`).  Archive errors as bce_hip_decompress_device, outputs
 * untouched. */
int bce_hip_decode_crc32(bce_hip_ctx *ctx, const uint8_t *archive, size_t len, size_t *decoded, uint32_t *crc);
/* bce_hip_decompress_device with the CRC-32 of the text beside it: taken on the device from the context's buffer before the copy
 * to the host is queued (`bce -d` on a version-2 container).  out == NULL: only the size is reported, *crc untouched. */
int bce_hip_decompress_device_crc32(bce_hip_ctx *ctx, const uint8_t *archive, size_t len, uint8_t *out, size_t cap, size_t *out_len,
                                    uint32_t *crc);

/* ---- extension: how often byte strings occur in the input, from the planes (kd_count.hip, fm_step.h) -------------------------
 * After bce_hip_build_planes the context holds a counting index of its input: the BWT of all cyclic rotations as a wavelet matrix
 * with a rank directory.  Backward search on it -- one last-to-first step per pattern byte, eight rank levels each -- counts the
 * rotations that start with a pattern: the CYCLIC count, the i in [0, n) with P[k] == T[(i + k) mod n] for all k < m.  Defined for
 * every length: the empty pattern occurs n times, a pattern longer than the text wraps around it.  (The count `bytes.count` would
 * give if it counted overlapping matches is this minus the occurrences that straddle the end of the text; bce_amd/api.py:
 * RankFile.count.)  npat patterns arrive concatenated: pattern p is patterns[offsets[p], offsets[p + 1]), npat + 1 offsets,
 * non-decreasing; counts[p] receives its count.
 * Valid from bce_hip_build_planes on for as long as the planes stand (through bce_hip_encode / _estimate / _scan and after them;
 * until the next load, bce_hip_set_bwt or decode); otherwise BCE_HIP_E_STATE with a bce_hip_last_error text.  Neither call changes
 * the context's compression state: an encode after a count gives the archive it would have given.  npat == 0: success, nothing
 * touched.  A null ctx, a null array with npat > 0, offsets that decrease: BCE_HIP_E_ARG. */
int bce_hip_count(bce_hip_ctx *ctx, const uint8_t *patterns, const uint64_t *offsets, uint32_t npat, uint64_t *counts);
/* The same with all three arrays in device memory of the context's device (offsets and counts 8-byte aligned).  Stream rule of
 * bce_hip_decompress_to_device: runs on the context's stream, complete on return; the memory must be ready when the call is made.
 * Decreasing offsets are found by the kernel (BCE_HIP_E_ARG after it has run; the counts are then undefined); that every offset
 * lies inside the patterns' buffer is the caller's to keep. */
int bce_hip_count_device(bce_hip_ctx *ctx, const void *d_patterns, const void *d_offsets, uint32_t npat, void *d_counts);
/* len bytes of the input the context holds, from position pos, to the host (the few bytes at the two ends of the text that turn a
 * cyclic count into a linear one, when the input came from device memory).  Valid as bce_hip_input_crc32; pos + len > n:
 * BCE_HIP_E_ARG. */
int bce_hip_input_bytes(bce_hip_ctx *ctx, uint64_t pos, size_t len, uint8_t *out);

/* ---- extension: WHERE byte strings occur in the input, from the planes and K1's suffix array (kd_locate.hip, fm_step.h) --------
 * Backward search ends at an interval [lo, hi) of the sorted rotations, and bce_hip_bwt leaves their order -- the suffix array,
 * 4 n bytes the depth-first tail of the enumeration needs anyway -- in device memory: the occurrences are sa[lo .. hi).  No samples.
 *   cyclic hits (flags == 0): the i in [0, n) with P[k] == T[(i + k) mod n] for all k < m: the set bce_hip_count counts.  Defined
 *     for m == 0 (every i) and m > n; in a periodic text every tied rotation is a hit.
 *   linear hits (BCE_HIP_LOCATE_LINEAR): those with i + m <= n, what an overlapping scan of the text finds; none for m > n.  The
 *     filter runs on the device.
 * Patterns arrive as for bce_hip_count.  The answer is CSR: hit_offsets[npat + 1], hit_offsets[0] == 0, pattern p owns
 * positions[hit_offsets[p] .. hit_offsets[p + 1]), ascending; hit_offsets is exact in both modes (its differences are the counts)
 * and *total (a host value) is its last word.
 * Overflow protocol: hit_offsets and *total are written whenever the call gets as far as the search.  positions == NULL with
 * cap == 0 is a sizing call and succeeds.  total > cap: BCE_HIP_E_OVERFLOW, hit_offsets and *total valid, no byte of positions
 * written.  One call gathers at most 2^31 - 1 cyclic rows (the sum of the patterns' cyclic counts, also in linear mode): beyond
 * that BCE_HIP_E_OVERFLOW with hit_offsets and *total exact, whatever cap is -- split the batch.
 * Valid while the planes stand (bce_hip_count's rule) AND the suffix array does: from bce_hip_build_planes after bce_hip_bwt,
 * through bce_hip_encode / _estimate / _scan / _count and after them, until the next load or decode.  After bce_hip_set_bwt:
 * BCE_HIP_E_STATE, "no suffix array behind an injected BWT".  Neither call changes the compression state.  npat == 0: success,
 * *total = 0, hit_offsets[0] = 0 where given.  A null ctx or total, a null array with npat > 0 (positions may be NULL only with
 * cap == 0), flag bits other than BCE_HIP_LOCATE_LINEAR, offsets that decrease: BCE_HIP_E_ARG.  Order of the checks, as for
 * bce_hip_count: ctx, total and flags first, then npat == 0, then the context's state (BCE_HIP_E_STATE wins over a null array), then
 * the arrays.  A sizing call and the full call that follows it each run the search. */
#define BCE_HIP_LOCATE_LINEAR 1u
int bce_hip_locate(bce_hip_ctx *ctx, const uint8_t *patterns, const uint64_t *offsets, uint32_t npat, uint32_t flags,
                   uint64_t *hit_offsets, uint32_t *positions, uint64_t cap, uint64_t *total);
/* The same with patterns, offsets, hit offsets and positions in device memory of the context's device (8-byte and 4-byte words
 * aligned as such); total stays a host pointer.  Stream rule and the kernel's offset check: as bce_hip_count_device. */
int bce_hip_locate_device(bce_hip_ctx *ctx, const void *d_patterns, const void *d_offsets, uint32_t npat, uint32_t flags,
                          void *d_hit_offsets, void *d_positions, uint64_t cap, uint64_t *total);

/* ---- extension: the same two questions with mismatches allowed (kd_near.hip, near_step.h) ---------------------------------------
 * T: the indexed text, n bytes, read circularly.  P: a pattern of m bytes.  The distance of P at position i in [0, n) is the Hamming
 * distance d(i) = #{ j < m : P[j] != T[(i + j) mod n] }.
 *   cyclic hits: the i with d(i) <= k.  Every i has exactly one distance and is counted once, under it.  Defined for every m:
 *     m == 0 gives all n positions at distance 0, k >= m gives all n positions, m > n wraps as it does for bce_hip_count.
 *   linear hits (BCE_HIP_LOCATE_LINEAR): those with i + m <= n, what a sliding window over the text finds; none for m > n.
 * 0 <= k <= BCE_HIP_NEAR_MAX_K and m <= BCE_HIP_NEAR_MAX_LEN: WORK bounds, not limits of any format (as BCE_HIP_MATCH_MAX_LEN);
 * outside them BCE_HIP_E_ARG.  The search is backward search that branches: two different strings of one length own disjoint row
 * intervals, so the hits are the disjoint union of the intervals of the strings within k mismatches of P that occur -- counts add
 * and nothing is found twice.  Its work grows with the number of such strings that occur, up to C(m, k) * 255^k on a text that holds
 * everything: that, on machines that are shared, is why k stops at 2 (DESIGN.md 4.17 has the figures).
 * Patterns arrive as for bce_hip_count.
 * bce_hip_count_near: counts[p * (k + 1) + d] = the cyclic hits of pattern p at distance exactly d, d = 0 .. k.  Cyclic only, as
 * bce_hip_count (the linear correction is the caller's, from the text's two ends: bce_amd/api.py: RankFile.count_near).  State,
 * order of the checks and npat == 0 as bce_hip_count, with k judged beside ctx; k == 0 gives bce_hip_count's counts.
 * bce_hip_locate_near: bce_hip_locate's protocol word for word -- the CSR answer (positions ascending within each pattern), the
 * sizing call (positions and dists NULL, cap 0), BCE_HIP_E_OVERFLOW with exact hit_offsets and *total when total > cap or the
 * batch's cyclic rows exceed 2^31 - 1, the validity (planes AND suffix array; BCE_HIP_E_STATE after bce_hip_set_bwt), the order of
 * the checks (k beside the flags), no change to the compression state -- plus dists[r], the distance of positions[r]; positions and
 * dists are given together or not at all.  k == 0 gives bce_hip_locate's positions.  npat <= 2^30 for this call (the distance
 * travels in the two low bits of the pattern's number through the sorts): more is BCE_HIP_E_ARG. */
#define BCE_HIP_NEAR_MAX_K 2u
#define BCE_HIP_NEAR_MAX_LEN 4096u
int bce_hip_count_near(bce_hip_ctx *ctx, const uint8_t *patterns, const uint64_t *offsets, uint32_t npat, uint32_t k, uint64_t *counts);
/* The same with all three arrays in device memory of the context's device.  Stream rule and the kernel's checks (decreasing
 * offsets, and here a pattern longer than BCE_HIP_NEAR_MAX_LEN): as bce_hip_count_device. */
int bce_hip_count_near_device(bce_hip_ctx *ctx, const void *d_patterns, const void *d_offsets, uint32_t npat, uint32_t k, void *d_counts);
int bce_hip_locate_near(bce_hip_ctx *ctx, const uint8_t *patterns, const uint64_t *offsets, uint32_t npat, uint32_t k, uint32_t flags,
                        uint64_t *hit_offsets, uint32_t *positions, uint8_t *dists, uint64_t cap, uint64_t *total);
/* The same with patterns, offsets, hit offsets, positions and distances in device memory of the context's device; total stays a
 * host pointer.  Stream rule and the kernel's checks: as bce_hip_count_near_device. */
int bce_hip_locate_near_device(bce_hip_ctx *ctx, const void *d_patterns, const void *d_offsets, uint32_t npat, uint32_t k, uint32_t flags,
                               void *d_hit_offsets, void *d_positions, void *d_dists, uint64_t cap, uint64_t *total);

/* ---- extension: the same two questions within k EDITS: substitutions, insertions and deletions (kd_edit.hip, edit_step.h) --------
 * T: the indexed text, n bytes, read circularly.  P: a pattern of m bytes.  0 <= k <= BCE_HIP_EDIT_MAX_K.
 * For a string S of l bytes the ANCHORED edit distance e(P, S) is the least number of substitutions, insertions and deletions that
 * turn P into S among the alignments in which P's first byte is aligned with S's first byte and P's last byte with S's last byte,
 * each of those two a match or a substitution, never an indel (what aligners do at the ends of a seed: an exact hit at i does not
 * also report i - 1 and i + 1 at distance 1):
 *   m == 0: e = 0 for l == 0, otherwise infinite.    m == 1: e = [P[0] != S[0]] for l == 1, otherwise infinite.
 *   m >= 2: e is infinite for l < 2, otherwise [P[0] != S[0]] + Lev(P[1 .. m-1), S[1 .. l-1)) + [P[m-1] != S[l-1]], Lev the plain
 *           Levenshtein distance.
 * For a position i in [0, n) let S(i, l) = T[(i + j) mod n], j < l, with l in [max(0, m - k), m + k].
 *   cyclic: E(i) = min over l of e(P, S(i, l)).  i is a hit when E(i) <= k; its distance is E(i), its length L(i) the smallest l
 *     that attains E(i).  m == 0 gives all n positions at distance 0 and length 0, k >= m gives every position, m > n wraps as it
 *     does for bce_hip_count.
 *   linear (BCE_HIP_LOCATE_LINEAR): the same with l restricted to i + l <= n BEFORE the minimum is taken: a position whose best cyclic
 *     alignment runs across the end of the text can still be a hit through a shorter or dearer one, at that one's distance and
 *     length.  P = "abcd", a text that ends in "abc" and starts with "d", k = 2: cyclic (n - 3, distance 0, length 4), linear
 *     (n - 3, distance 2, length 3).
 * Every position is reported at most once per pattern.  k == 0 gives bce_hip_count / bce_hip_locate, every length m.  For m <= 1 no
 * indel is possible and the answer is bce_hip_count_near's; for m == 2 the only indel is an insertion between the two bytes.
 * k <= BCE_HIP_EDIT_MAX_K and m <= BCE_HIP_EDIT_MAX_LEN are WORK bounds in the sense of BCE_HIP_NEAR_MAX_LEN; outside them
 * BCE_HIP_E_ARG.  npat <= BCE_HIP_EDIT_MAX_PATTERNS for all four calls (a candidate's edits and length travel in the four low bits
 * of the pattern's number through the sorts): more is BCE_HIP_E_ARG.
 * The search enumerates edit scripts by backward search and finds CANDIDATES: different scripts reach one string and strings of
 * different lengths nest, so a position is found many times, and the answer is the least (distance, length) per position, reduced
 * on the device through the suffix array.  Hence:
 *   - both calls need the planes AND the suffix array, counting included: BCE_HIP_E_STATE after bce_hip_set_bwt, as bce_hip_locate;
 *   - both take the flags: the linear restriction is part of the reduce, not a correction of the caller's;
 *   - what one call bounds is the batch's CANDIDATE rows, not its hits: more than 2^31 - 1 of them is BCE_HIP_E_OVERFLOW with
 *     nothing written (no offsets, *total = 0), whatever cap is;
 *   - a sizing call costs a whole search: the hits are only known after the reduce.
 * Patterns arrive as for bce_hip_count.
 * bce_hip_count_edit: counts[p * (k + 1) + d] = the hits of pattern p at distance exactly d, d = 0 .. k.  Order of the checks: ctx,
 * k, flags and npat's cap first, then npat == 0, then the state, then the arrays.
 * bce_hip_locate_edit: bce_hip_locate_near's protocol word for word -- the CSR answer (positions ascending within each pattern), the
 * sizing call (positions, lens and dists NULL, cap 0), BCE_HIP_E_OVERFLOW with exact hit_offsets and *total when total > cap and
 * then no byte of positions, lens or dists written, the order of the checks, no change to the compression state -- plus lens[r] =
 * L(positions[r]); positions, lens and dists are given together or not at all. */
#define BCE_HIP_EDIT_MAX_K 2u
#define BCE_HIP_EDIT_MAX_LEN 4096u
#define BCE_HIP_EDIT_MAX_PATTERNS (1u << 28)
int bce_hip_count_edit(bce_hip_ctx *ctx, const uint8_t *patterns, const uint64_t *offsets, uint32_t npat, uint32_t k, uint32_t flags,
                       uint64_t *counts);
/* The same with all three arrays in device memory of the context's device.  Stream rule and the kernel's checks (decreasing
 * offsets, a pattern longer than BCE_HIP_EDIT_MAX_LEN): as bce_hip_count_near_device. */
int bce_hip_count_edit_device(bce_hip_ctx *ctx, const void *d_patterns, const void *d_offsets, uint32_t npat, uint32_t k, uint32_t flags,
                              void *d_counts);
int bce_hip_locate_edit(bce_hip_ctx *ctx, const uint8_t *patterns, const uint64_t *offsets, uint32_t npat, uint32_t k, uint32_t flags,
                        uint64_t *hit_offsets, uint32_t *positions, uint16_t *lens, uint8_t *dists, uint64_t cap, uint64_t *total);
/* The same with patterns, offsets, hit offsets, positions, lengths (2-byte words) and distances in device memory of the context's
 * device; total stays a host pointer.  Stream rule and the kernel's checks: as bce_hip_count_edit_device. */
int bce_hip_locate_edit_device(bce_hip_ctx *ctx, const void *d_patterns, const void *d_offsets, uint32_t npat, uint32_t k, uint32_t flags,
                               void *d_hit_offsets, void *d_positions, void *d_lens, void *d_dists, uint64_t cap, uint64_t *total);

/* ---- extension: the same two questions for patterns of byte CLASSES (kd_classes.hip, class_step.h) ------------------------------
 * T: the indexed text, n bytes, read circularly.  A pattern P is m classes S_0 .. S_(m-1); every class is a set of bytes: a wildcard,
 * a range, both cases of a letter, one byte.
 *   layout: a class is 256 bits in 8 uint32_t words; byte c is in S iff bit c & 31 of word c >> 5 is set.  masks holds
 *     8 * offsets[npat] words; offsets has npat + 1 entries counted in CLASSES, as the other batch calls count bytes.
 *   cyclic hits: the i in [0, n) with T[(i + j) mod n] in S_j for all j < m.  m == 0 matches all n positions; an empty class
 *     matches nothing; m > n wraps as it does for bce_hip_count.
 *   linear hits (BCE_HIP_LOCATE_LINEAR): those with i + m <= n, what a sliding window over the text finds; none for m > n.
 * The search is backward search that branches at every class of two members or more (a WIDE class): two different strings of one
 * length own disjoint row intervals, so the hits are the disjoint union of the intervals of the strings of P's language that occur.
 * The WORK of a pattern is fixed by the text and the pattern, not by the order of the walk:
 *   nodes(P) = #{ (j, s) : 1 <= j <= m, s a string of j bytes with s[t] in S_(m-j+t) for all t, s occurs in the circular text },
 * the non-root nodes of the right-to-left search tree that have rows.  `.{8}` asks for every distinct 8-gram of the text: so every
 * call takes a BUDGET, max_nodes per pattern (0: BCE_HIP_CLASS_DEFAULT_NODES; above BCE_HIP_CLASS_MAX_NODES: BCE_HIP_E_ARG).  Both are
 * 2^16: a batch of 4096 patterns that all exhaust that budget was measured at 0.9 to 1.1 s on an MI355X, four times the budget at
 * four times that -- the cap keeps one call on a shared machine at about a second, and the default cannot exceed it.
 * Both values are PROVISIONAL: they follow the walk's measured cost per node and rise when that falls.
 *   nodes(P) <= max_nodes: status[p] = 0, work[p] = nodes(P) exactly, the answer is complete.
 *   otherwise: status[p] = BCE_HIP_CLASS_OVER, the count is 0 and the locate's segment empty, work[p] is some value > max_nodes.
 *     The walk stops within one frame's expansion and one finish chain of crossing the budget -- at most 256 m further steps;
 *     it never walks the whole tree first.  One pattern over budget fails neither the call nor the other patterns.
 * WORK bounds, as BCE_HIP_NEAR_MAX_LEN: m <= BCE_HIP_CLASS_MAX_LEN classes, of which at most BCE_HIP_CLASS_MAX_WIDE are wide (the
 * only ones that need a frame of the walk's stack); more, or offsets that decrease: BCE_HIP_E_ARG, found by the kernel in both forms
 * of the calls (after it has run; the outputs are then undefined).
 * bce_hip_count_classes: counts[p] = the cyclic hits of pattern p.  Cyclic only, as bce_hip_count (the linear correction is the
 * caller's, from the text's two ends: bce_amd/api.py: class_linear_counts).  work may be NULL.  State, order of the checks and
 * npat == 0 as bce_hip_count, with max_nodes judged beside ctx.  A pattern of one-member classes gives bce_hip_count's count.
 * bce_hip_locate_classes: bce_hip_locate's protocol word for word -- the CSR answer (positions ascending within each pattern), the
 * sizing call (positions NULL, cap 0), BCE_HIP_E_OVERFLOW with exact hit_offsets and *total when total > cap or the batch's cyclic
 * rows exceed 2^31 - 1, the validity (planes AND suffix array; BCE_HIP_E_STATE after bce_hip_set_bwt), the order of the checks
 * (max_nodes beside the flags), no change to the compression state -- plus status[p], written whenever hit_offsets is.  A pattern
 * of one-member classes gives bce_hip_locate's positions. */
#define BCE_HIP_CLASS_MAX_LEN 4096u
#define BCE_HIP_CLASS_MAX_WIDE 64u
#define BCE_HIP_CLASS_DEFAULT_NODES (1u << 16)
#define BCE_HIP_CLASS_MAX_NODES (1u << 16)
#define BCE_HIP_CLASS_OVER 1u
int bce_hip_count_classes(bce_hip_ctx *ctx, const uint32_t *masks, const uint64_t *offsets, uint32_t npat, uint32_t max_nodes, uint64_t *counts,
                          uint64_t *work, uint32_t *status);
/* The same with every array in device memory of the context's device (d_work may be NULL).  Stream rule: as bce_hip_count_device. */
int bce_hip_count_classes_device(bce_hip_ctx *ctx, const void *d_masks, const void *d_offsets, uint32_t npat, uint32_t max_nodes, void *d_counts,
                                 void *d_work, void *d_status);
int bce_hip_locate_classes(bce_hip_ctx *ctx, const uint32_t *masks, const uint64_t *offsets, uint32_t npat, uint32_t max_nodes, uint32_t flags,
                           uint64_t *hit_offsets, uint32_t *status, uint32_t *positions, uint64_t cap, uint64_t *total);
/* The same with masks, offsets, hit offsets, verdicts and positions in device memory of the context's device; total stays a host
 * pointer.  Stream rule: as bce_hip_count_device. */
int bce_hip_locate_classes_device(bce_hip_ctx *ctx, const void *d_masks, const void *d_offsets, uint32_t npat, uint32_t max_nodes, uint32_t flags,
                                  void *d_hit_offsets, void *d_status, void *d_positions, uint64_t cap, uint64_t *total);

/* ---- extension: the longest matches of a SECOND buffer in the input (kd_match.hip, fm_step.h) -----------------------------------
 * The matching statistics of a query Q (q bytes, 1 <= q <= 2^31 - 1) against the text T (the n bytes the context indexed).  For
 * every END position i in [0, q):
 *   len[i]  the largest l with 0 <= l <= min(max_len, i + 1) such that Q[i - l + 1 .. i] occurs in T;
 *   pos[i]  the start in T of ONE such occurrence (which one is not specified: the tied rotations of a periodic text stand in any
 *           order), 0xFFFFFFFF where len[i] == 0.
 *   cyclic (flags == 0): "occurs" in the circular text, as bce_hip_count defines it; l may exceed n on a periodic text.
 *   linear (BCE_HIP_MATCH_LINEAR): an occurrence that starts at a p with p + l <= n, and pos[i] is such a p.
 * In both modes len[i + 1] <= len[i] + 1, and a match that is cut short at max_len is reported as max_len.  max_len is a WORK bound
 * per end position, 1 .. BCE_HIP_MATCH_MAX_LEN, not a limit of any format: a lane extends its match by at most that many bytes.
 * Backward search from each end position, one lane each, with the step bce_hip_count runs; linear mode reads suffix-array entries
 * only while an interval holds fewer rows than the match has bytes.
 * pos_out may be NULL.  Cyclic lengths without positions need only the planes (they work after bce_hip_set_bwt); positions, and
 * everything in linear mode, need the suffix array by bce_hip_locate's rule, otherwise BCE_HIP_E_STATE in its words.  Valid while
 * the planes stand (bce_hip_count's rule); no call here changes the compression state: an encode after a match gives the archive
 * of a fresh context.  q == 0: success, nothing launched.  A null ctx, a flag bit other than BCE_HIP_MATCH_LINEAR, a max_len
 * outside 1 .. BCE_HIP_MATCH_MAX_LEN, q >= 2^31: BCE_HIP_E_ARG before any device call; then the state; then a null query or
 * len_out: BCE_HIP_E_ARG. */
#define BCE_HIP_MATCH_LINEAR 1u
#define BCE_HIP_MATCH_MAX_LEN 4096u
int bce_hip_match(bce_hip_ctx *ctx, const uint8_t *query, uint64_t q, uint32_t max_len, uint32_t flags, uint32_t *len_out,
                  uint32_t *pos_out);
/* The same with the query, the lengths and the positions (d_pos may be NULL) in device memory of the context's device, the two
 * outputs 4-byte aligned.  Stream rule: as bce_hip_count_device. */
int bce_hip_match_device(bce_hip_ctx *ctx, const void *d_query, uint64_t q, uint32_t max_len, uint32_t flags, void *d_len,
                         void *d_pos);
/* *covered = the number of j in [0, q) for which some i >= j has len[i] >= min_len and i - len[i] + 1 <= j: the size of the union of
 * all matches of min_len bytes or more, i.e. how many bytes of the query lie in strings of at least min_len bytes that occur in
 * the text.  The search runs with max_len = min_len (1 .. BCE_HIP_MATCH_MAX_LEN), which is enough: the windows of min_len bytes
 * that end inside a longer match cover it.  Search and reduction run on the device; 8 bytes come back.  Modes, state and refusals
 * as bce_hip_match without positions; a null covered: BCE_HIP_E_ARG; q == 0: *covered = 0. */
int bce_hip_coverage(bce_hip_ctx *ctx, const uint8_t *query, uint64_t q, uint32_t min_len, uint32_t flags, uint64_t *covered);
/* The same with the query in device memory; covered stays a host pointer. */
int bce_hip_coverage_device(bce_hip_ctx *ctx, const void *d_query, uint64_t q, uint32_t min_len, uint32_t flags, uint64_t *covered);

/* ---- extension: what the input holds by ITSELF: LCP array, k-gram classes, longest repeat (kd_lcp.hip, lcp_step.h) -------------
 * Everything here is about the CIRCULAR text, as bce_hip_count's cyclic mode and the coder see it: rotation a of the n bytes T is
 * T[(a + j) mod n], j = 0, 1, ...  The LINEAR variant is the section "what the input REPEATS of itself" below (bce_hip_lpf): the
 * longest repeat of the linear text is not a maximum over adjacent rows (a middle row that starts near the text's end truncates
 * the pairs with both of its neighbours), so it is no by-product of this array; its neighbours are the nearest rows that start
 * earlier in the text, and it is the largest lpf[i].
 *   lcp[0] = 0, and for 1 <= r < n lcp[r] = the largest l <= max_len with T[(sa[r-1] + j) mod n] == T[(sa[r] + j) mod n] for all
 *   j < l, sa = the sorted rotations (what bce_hip_locate reads).  There is NO cap at n: two equal rotations of a periodic text
 *   give max_len.  So the capped array is a function of the text alone -- rows tied to max_len bytes all carry max_len among
 *   themselves, in whatever order the sort left them.  max_len is a WORK bound per row, 1 .. BCE_HIP_MATCH_MAX_LEN, not a limit of
 *   any format; one lane per row compares eight bytes at a time, byte by byte across the text's end.
 * State: the suffix array by bce_hip_locate's rule AND the loaded text (not behind bce_hip_set_bwt, not after a decode took the
 * buffers): otherwise BCE_HIP_E_STATE in bce_hip_locate's words.  A text of one byte has no array: lcp = [0].  No call here
 * changes the compression state or writes a stage's buffers, and nothing is cached from one call to the next: each call runs
 * its own pass.  A null ctx, a max_len outside 1 .. BCE_HIP_MATCH_MAX_LEN: BCE_HIP_E_ARG before any device call; then the state;
 * then a null output: BCE_HIP_E_ARG.  A refused call leaves its outputs untouched. */
int bce_hip_lcp(bce_hip_ctx *ctx, uint32_t max_len, uint32_t *lcp_out);
/* The same into n words of device memory of the context's device, 4-byte aligned.  Stream rule: as bce_hip_count_device. */
int bce_hip_lcp_device(bce_hip_ctx *ctx, uint32_t max_len, void *d_lcp);
/* The cyclic k-grams of the text, for nk <= BCE_HIP_KGRAMS_MAX values of k in 0 .. BCE_HIP_MATCH_MAX_LEN (host arrays), from ONE
 * LCP pass bounded by the largest k (at least 1).  For a k, a class is a maximal run of rows [s, e) with lcp[r] >= k for
 * s < r < e: the rotations that start with one k-gram w, e - s = N(w) its occurrences in the circular text (k > n wraps around;
 * k = 0: one class of n rows).  Per k:
 *   distinct   the classes, i.e. the distinct k-grams;       once       those that occur once;
 *   nlogn_q24  S_k = the sum over the classes of N * L(N), L = the Q24 integer log2 of bce_hip_cost_q24 (L(N) = cost_q24(1, N)):
 *              a uint64_t sum, exact and independent of the order, below n * L(n) < 2^60.  For the circular text the order-k
 *              empirical entropy is n * H_k = S_k - S_(k+1), in units of 2^-24 bit;
 *   max_count  the largest class;  max_pos  the start of a rotation of the lowest-row class that reaches it (sa[s]; which of the
 *              tied rotations of a periodic text that is, is not specified).
 * Reduced on the device, block-wise and without atomics; 32 bytes per k come back.  n == 1: every k gives {1, 1, 0, 1, 0}.
 * nk == 0: success, nothing launched.  A null ctx, nk > BCE_HIP_KGRAMS_MAX, a null ks, a k above BCE_HIP_MATCH_MAX_LEN:
 * BCE_HIP_E_ARG before any device call; then the state; then a null out: BCE_HIP_E_ARG. */
#define BCE_HIP_KGRAMS_MAX 64u
typedef struct bce_hip_kgram {
  uint64_t distinct, once, nlogn_q24;
  uint32_t max_count, max_pos;
} bce_hip_kgram;
int bce_hip_kgrams(bce_hip_ctx *ctx, const uint32_t *ks, uint32_t nk, bce_hip_kgram *out);
/* The longest repeat of the circular text: *len = the largest lcp[r] at bound max_len, *pos_a = sa[r - 1] and *pos_b = sa[r] of
 * the lowest row r that reaches it: two rotations that agree on *len bytes.  *len == max_len means "max_len bytes or more".
 * *len == 0 (no byte occurs twice; n == 1 always): there is no pair, both positions are 0xFFFFFFFF.  State and refusals as
 * bce_hip_lcp; all three outputs are required. */
int bce_hip_longest_repeat(bce_hip_ctx *ctx, uint32_t max_len, uint32_t *len, uint32_t *pos_a, uint32_t *pos_b);

/* ---- extension: the MOST FREQUENT k-grams of the input, as a list (kd_lcp.hip, top_step.h) ---------------------------------------
 * For one k in 0 .. BCE_HIP_MATCH_MAX_LEN, the classes of bce_hip_kgrams (circular text: k = 0 gives one class of n rows, k > n wraps
 * around, n == 1 gives the one class {1, 0, 0} for every k) ordered by size descending and, among equal sizes, by first row
 * ascending.  Rows are sorted rotations, so the tie order is the lexicographic order of the k-grams as byte strings: the order,
 * every count and every row are a function of the text alone.  The first min(limit, distinct) classes are returned:
 *   out[e].count  N(w);    out[e].row  the class's first row s;    out[e].pos  sa[s], the start of ONE occurrence (which of the tied
 *                 rotations of a periodic text it names is not specified; 0 for n == 1);
 *   bytes[e * k .. e * k + k)  T[(pos + j) mod n], the k-gram itself.  bytes may be NULL: the bytes are not wanted.  With bytes
 *                 non-NULL, bytes_cap must be at least limit * k: there is no sizing call.  out has room for limit entries.
 *   *found        the entries written;    *distinct (may be NULL)  the classes, bce_hip_kgram.distinct;
 *   size_hist[b]  (may be NULL) the classes with floor(log2 N) = b: the coarse frequency spectrum the selection computes anyway.
 * Selected on the device: the sizes are binned, the host picks the largest bin t with at least min(limit, distinct) classes at or
 * above it, those classes -- their number is known exactly, the buffers are sized by it and not by n -- are compacted in row order,
 * sorted stably on the size bits that can differ, and the first entries gathered with their bytes.  When every class lies in one
 * bin (all k-grams distinct, say) every class is a candidate.  Own LCP pass bounded by max(k, 1); nothing is cached; only buffers
 * of the feature's own are written and no compression state changes.
 * A null ctx, k > BCE_HIP_MATCH_MAX_LEN, a limit outside 1 .. BCE_HIP_TOP_MAX, a null found, bytes with bytes_cap < limit * k:
 * BCE_HIP_E_ARG (bce_hip_last_error has the words) before any device call; then the state, as bce_hip_kgrams; then a null out:
 * BCE_HIP_E_ARG.  A refused call leaves its outputs untouched. */
#define BCE_HIP_TOP_MAX (1u << 20)
typedef struct bce_hip_top_kgram {
  uint32_t count, row, pos;
} bce_hip_top_kgram;
int bce_hip_top_kgrams(bce_hip_ctx *ctx, uint32_t k, uint32_t limit, bce_hip_top_kgram *out, uint8_t *bytes, uint64_t bytes_cap,
                       uint32_t *found, uint64_t *distinct, uint64_t size_hist[32]);
/* The same into device memory of the context's device (d_out 4-byte aligned); found, distinct and size_hist stay host pointers.
 * Stream rule: as bce_hip_count_device. */
int bce_hip_top_kgrams_device(bce_hip_ctx *ctx, uint32_t k, uint32_t limit, void *d_out, void *d_bytes, uint64_t bytes_cap,
                              uint32_t *found, uint64_t *distinct, uint64_t size_hist[32]);

/* ---- extension: the MAXIMAL REPEATS of the input, as a list (kd_maxrep.hip, maxrep_step.h) ---------------------------------------
 * Which strings the circular text repeats, how long they are and how often they occur.  lcp: the array of bce_hip_lcp at bound
 * max_len; bw[r] = T[(sa[r] + n - 1) mod n].  A row r >= 1 with l = lcp[r] >= 1 lies in the LCP interval [p, q): p the nearest row
 * above with lcp[p] < l, q the nearest row below with lcp[q] < l, or n.  The interval is the class of one l-gram w with q - p >= 2
 * cyclic occurrences that are followed by at least two different bytes (for l < max_len); w is a MAXIMAL repeat when bw[p .. q) holds
 * at least two different bytes as well.  Each interval is reported once, by the lowest of its rows that carry l.
 *   out[e].len    l; len == max_len means "max_len bytes or more" (as bce_hip_longest_repeat's *len == max_len);
 *   out[e].count  q - p;    out[e].row  p;    out[e].pos  sa[p], the start of ONE occurrence (which of tied rotations is not specified).
 * len, count and row are functions of the text and max_len alone.  Ordered by a weight, descending, and among equal weights by the
 * reporting row ascending (for BY_LEN and BY_COUNT that is the lexicographic order of the strings):
 *   BCE_HIP_MAXREP_BY_LEN  (len << 31) | count;   BCE_HIP_MAXREP_BY_COUNT  (count << 13) | len;   BCE_HIP_MAXREP_BY_GAIN  len * (count - 1).
 * The first min(limit, total) repeats with len >= min_len are returned; info->found is their number, info->total and info->capped
 * count all of them (capped: those with len == max_len), info->bwt_runs = 1 + #{1 <= r < n : bw[r] != bw[r - 1]} is the number of
 * runs of the BWT.  A text of one byte, or one without repeats: found = total = 0, nothing is written to out.
 *   bytes (may be NULL)  bytes[e * bytes_per + j] = T[(pos + j) mod n] for j < min(len, bytes_per), the rest of the slot zero;
 *                        bytes_per <= 4096 and bytes_cap >= limit * bytes_per.  bytes_per == 0: as NULL.
 * Own LCP pass; nothing is cached; only buffers of the feature's own (and the LCP and tree buffers of bce_hip_lcp / _lpf) are
 * written and no compression state changes.
 * A null ctx, 1 <= min_len <= max_len <= BCE_HIP_MATCH_MAX_LEN violated, an unknown order, a limit outside 1 .. BCE_HIP_TOP_MAX, a
 * null info, bytes_per > 4096, bytes with bytes_cap < limit * bytes_per: BCE_HIP_E_ARG (bce_hip_last_error has the words) before any
 * device call; then the state, as bce_hip_top_kgrams; then a null out: BCE_HIP_E_ARG.  A refused call leaves its outputs untouched. */
#define BCE_HIP_MAXREP_BY_LEN 0u
#define BCE_HIP_MAXREP_BY_COUNT 1u
#define BCE_HIP_MAXREP_BY_GAIN 2u
typedef struct bce_hip_maxrep {
  uint32_t len, count, row, pos;
} bce_hip_maxrep;
typedef struct bce_hip_maxrep_info {
  uint64_t total;  /* maximal repeats with len >= min_len at this bound */
  uint64_t capped; /* those of them with len == max_len */
  uint64_t bwt_runs;
  uint32_t found, reserved;
} bce_hip_maxrep_info;
int bce_hip_maximal_repeats(bce_hip_ctx *ctx, uint32_t min_len, uint32_t max_len, uint32_t order, uint32_t limit, bce_hip_maxrep *out,
                            uint8_t *bytes, uint32_t bytes_per, uint64_t bytes_cap, bce_hip_maxrep_info *info);
/* The same into device memory of the context's device (d_out 4-byte aligned); info stays a host pointer.  Stream rule: as
 * bce_hip_count_device. */
int bce_hip_maximal_repeats_device(bce_hip_ctx *ctx, uint32_t min_len, uint32_t max_len, uint32_t order, uint32_t limit, void *d_out,
                                   void *d_bytes, uint32_t bytes_per, uint64_t bytes_cap, bce_hip_maxrep_info *info);

/* ---- extension: a second buffer as a DELTA against the input: parse and patch (kd_parse.hip, parse_step.h) ----------------------
 * T: the n bytes the context indexed.  Q: a query of q bytes, 0 <= q < 2^31.  1 <= min_len <= max_len <= BCE_HIP_MATCH_MAX_LEN.
 * len[i], pos[i]: the LINEAR matching statistics of Q at bound max_len, exactly what bce_hip_match_device gives with
 * BCE_HIP_MATCH_LINEAR and positions.  The parse is the chain
 *     e = q - 1;  while e >= 0:  len[e] >= min_len ?  a copy of len[e] bytes from T[pos[e] ..], it covers Q[e - len[e] + 1 .. e], e -= len[e]
 *                                                  :  the literal byte Q[e], e -= 1
 * (from the right, because the index extends matches to the left: the lengths by END position are what exists).  The phrases
 * come out in ascending query order, neighbouring literal bytes merged into one maximal run, as two streams: nops ops and nlits
 * literal bytes in query order.  An op with src == BCE_HIP_OP_LITERAL stands for the next len bytes of the literal stream, any other
 * for T[src .. src + len).  Which occurrence src names is not specified (as pos[i]); everything else about the output is unique.
 * For min_len == 1 no parse of Q into substrings of T of at most max_len bytes and single literal bytes has fewer phrases, every
 * literal byte counted as one; for a larger min_len that does not hold (a short copy may save a literal).
 * The search costs up to q * max_len lane steps (a wave runs as long as its longest lane), so max_len is the caller's to choose.
 * info (a host pointer, required) is written whenever the call gets as far as the chain: nlits + copied == q, nops - ncopies is the
 * number of literal runs.  ops == NULL and lits == NULL with both caps 0: a sizing call, which succeeds.  Otherwise nops > ops_cap
 * or nlits > lits_cap: BCE_HIP_E_OVERFLOW with info exact and no byte of either output written.  A sizing call and the full call
 * that follows it each run the search.  State and refusals as bce_hip_match with positions (BCE_HIP_E_STATE in bce_hip_locate's
 * words behind an injected BWT); no call here changes the compression state or writes a stage's buffers: an encode after a parse
 * gives the archive of a fresh context.  q == 0: success, info all zero, nothing launched.  A null ctx or info, bounds outside
 * 1 <= min_len <= max_len <= BCE_HIP_MATCH_MAX_LEN, q >= 2^31: BCE_HIP_E_ARG before any device call; then the state; then a null
 * query, or a null output with a cap above 0: BCE_HIP_E_ARG. */
#define BCE_HIP_OP_LITERAL 0xFFFFFFFFu
typedef struct bce_hip_op {
  uint32_t len, src;
} bce_hip_op;
typedef struct bce_hip_parse_info {
  uint64_t nops, nlits, ncopies, copied;
} bce_hip_parse_info;
int bce_hip_parse(bce_hip_ctx *ctx, const uint8_t *query, uint64_t q, uint32_t min_len, uint32_t max_len, bce_hip_op *ops,
                  uint64_t ops_cap, uint8_t *lits, uint64_t lits_cap, bce_hip_parse_info *info);
/* The same with the query, the ops (4-byte aligned) and the literal bytes in device memory of the context's device; info stays a
 * host pointer.  Stream rule: as bce_hip_count_device. */
int bce_hip_parse_device(bce_hip_ctx *ctx, const void *d_query, uint64_t q, uint32_t min_len, uint32_t max_len, void *d_ops,
                         uint64_t ops_cap, void *d_lits, uint64_t lits_cap, bce_hip_parse_info *info);
/* The bytes that nops ops and nlits literal bytes describe over T, into out: ANY well-formed list, not only bce_hip_parse's; a
 * copy's len may be anything from 1 to 2^31 - 1, copies may overlap and repeat.  Needs the loaded text only (no planes, no suffix
 * array): valid from a load until a decode or bce_hip_set_bwt takes the text away, otherwise BCE_HIP_E_STATE.  A validation pass
 * on the device comes first: an op with len == 0, a copy with src + len > n, literal lengths that do not add up to exactly nlits,
 * a total of 2^31 bytes or more: BCE_HIP_E_ARG with the reason in bce_hip_last_error, nothing copied, out untouched.  Then
 * *out_len = the total; total > cap: BCE_HIP_E_OVERFLOW, out untouched.  out == NULL with cap == 0 sizes and validates.  nops == 0:
 * *out_len = 0 (nlits must be 0).  The copy is divided by output bytes, not by ops.  A null ctx or out_len, nops >= 2^31 (every
 * op holds a byte), a null ops with nops > 0 or lits with nlits > 0, a null out with cap > 0: BCE_HIP_E_ARG before any device call. */
int bce_hip_patch(bce_hip_ctx *ctx, const bce_hip_op *ops, uint64_t nops, const uint8_t *lits, uint64_t nlits, uint8_t *out,
                  uint64_t cap, uint64_t *out_len);
/* The same with the ops (4-byte aligned), the literal bytes and the result (any alignment) in device memory; out_len stays a host
 * pointer.  d_out may not overlap the other two.  Stream rule: as bce_hip_count_device. */
int bce_hip_patch_device(bce_hip_ctx *ctx, const void *d_ops, uint64_t nops, const void *d_lits, uint64_t nlits, void *d_out,
                         uint64_t cap, uint64_t *out_len);
/* Test hook (tests/test_gpu_parse_scans.py), valid in any state of the context: the parse alone -- bce_hip_parse_device without
 * its search -- on q lengths, positions (d_pos may be NULL: every copy's src is 0) and query bytes of the caller's, with the launches
 * and launch geometry of the real call (which runs the same function): blocks of 2048 positions, one workgroup that walks the
 * blocks' sums 256 at a time.  It requires only d_len[i] <= i + 1, NOT lengths up to BCE_HIP_MATCH_MAX_LEN, so a jump can cross
 * any number of blocks.  Writes only the feature's par_* buffers and the two outputs; sizing, overflow and info as bce_hip_parse.
 * A null ctx or info, q >= 2^31, a min_len outside 1 .. BCE_HIP_MATCH_MAX_LEN, q > 0 with a null d_len or d_query, a null output
 * with a cap above 0: BCE_HIP_E_ARG before any device call. */
int bce_hip_parse_of_lengths_device(bce_hip_ctx *ctx, const void *d_len, const void *d_pos, const void *d_query, uint64_t q,
                                    uint32_t min_len, void *d_ops, uint64_t ops_cap, void *d_lits, uint64_t lits_cap,
                                    bce_hip_parse_info *info);

/* ---- extension: what the input REPEATS of itself: longest previous factors and the LZ77 factorisation (kd_self.hip, lpf_step.h) ----
 * T: the n bytes the context indexed, taken as LINEAR.  1 <= min_len <= max_len <= BCE_HIP_MATCH_MAX_LEN.
 *   lpf[i]  the largest l <= min(max_len, n - i) such that some j < i has T[j .. j + l) == T[i .. i + l); the source may overlap the
 *           destination; lpf[0] = 0.  max_len is a work bound per position, as for bce_hip_lcp.
 *   src[i]  one such j, 0xFFFFFFFF where lpf[i] == 0.  Which j it names is not specified (as pos[i] of the match); everything else
 *           is a function of the text alone.
 * With sa the sorted rotations and sa[r] = i, the candidates are the nearest row above r and the nearest row below r whose sa
 * value is smaller than i (all nearest smaller values over sa, an implicit min-tree: O(log n) loads per row and side, 4 n bytes of
 * the feature's own); lpf[i] is the longer of the two common prefixes at the bound min(max_len, n - i), with which no compare wraps.
 * The self-parse is the chain
 *     s = 0;  while s < n:  lpf[s] >= min_len ?  a copy of lpf[s] bytes from T[src[s] ..], s += lpf[s]  :  the literal byte T[s], s += 1
 * and comes out as bce_hip_parse gives a parse: ops in ascending text order, neighbouring literal bytes merged into maximal runs
 * with src == BCE_HIP_OP_LITERAL, plus the literal bytes; info as there, nlits + copied == n.  Every copy has src < its
 * destination, so the list decodes from left to right WITHOUT T (a copy may overlap its own output: byte by byte); bce_hip_patch
 * over T gives T back as well.  For min_len == 1 no parse of T into earlier-occurring substrings of at most max_len bytes and
 * single literal bytes has fewer phrases (ncopies + nlits): the greedy LZ77 factorisation, z = ncopies + nlits.
 * State: as bce_hip_lcp (the suffix array AND the loaded text, else BCE_HIP_E_STATE in bce_hip_locate's words).  n == 1: lpf = [0],
 * one literal op, no array is read.  No call here changes the compression state or writes a stage's buffers; nothing is cached.
 * Sizing call, BCE_HIP_E_OVERFLOW and info exactly as bce_hip_parse.  A null ctx (or info), bounds outside 1 <= (min_len <=)
 * max_len <= BCE_HIP_MATCH_MAX_LEN, a null output with a cap above 0: BCE_HIP_E_ARG before any device call; then the state; then a
 * null lpf_out: BCE_HIP_E_ARG.  src_out may be NULL: the sources are not wanted.  A refused call leaves its outputs untouched. */
int bce_hip_lpf(bce_hip_ctx *ctx, uint32_t max_len, uint32_t *lpf_out, uint32_t *src_out);
/* The same into n words each of device memory of the context's device, 4-byte aligned (d_src may be NULL).  Stream rule: as
 * bce_hip_count_device. */
int bce_hip_lpf_device(bce_hip_ctx *ctx, uint32_t max_len, void *d_lpf, void *d_src);
int bce_hip_self_parse(bce_hip_ctx *ctx, uint32_t min_len, uint32_t max_len, bce_hip_op *ops, uint64_t ops_cap, uint8_t *lits,
                       uint64_t lits_cap, bce_hip_parse_info *info);
/* The same with the ops (4-byte aligned) and the literal bytes in device memory; info stays a host pointer. */
int bce_hip_self_parse_device(bce_hip_ctx *ctx, uint32_t min_len, uint32_t max_len, void *d_ops, uint64_t ops_cap, void *d_lits,
                              uint64_t lits_cap, bce_hip_parse_info *info);
/* Test hooks (tests/test_gpu_nsv.py, tests/test_gpu_self_scans.py), valid in any state of the context, with the launches and launch
 * geometry of the real calls (which run the same functions); they write only the feature's slf_* buffers (the second also
 * kd_parse's par_*) and their outputs.
 * nsv: d_psv[r] / d_nsv[r] = the nearest row above / below r with d_vals[row] < d_vals[r], STRICTLY (equal values are never
 * smaller), 0xFFFFFFFF where there is none; any n words, 1 <= n < 2^31.  A null pointer, n == 0 or n >= 2^31: BCE_HIP_E_ARG.
 * self_parse_of_lpf: the chain alone on n lengths, sources (d_src may be NULL: every copy's src is 0) and text bytes of the
 * caller's.  It requires only d_lpf[i] <= n - i, so a jump can cross any number of blocks.  Arguments as
 * bce_hip_parse_of_lengths_device. */
int bce_hip_nsv_device(bce_hip_ctx *ctx, const void *d_vals, uint32_t n, void *d_psv, void *d_nsv);
int bce_hip_self_parse_of_lpf_device(bce_hip_ctx *ctx, const void *d_lpf, const void *d_src, const void *d_text, uint64_t n,
                                     uint32_t min_len, void *d_ops, uint64_t ops_cap, void *d_lits, uint64_t lits_cap,
                                     bce_hip_parse_info *info);

/* ---- extension: the SUFFIX ARRAY of a buffer as a product, and a checker for one (k1_bwt.hip, kd_sufsort.hip) --------------------
 * T: n bytes, 0 < n < 2^31 - 1, taken as LINEAR.  sa[r], r < n, is the start of the r-th smallest suffix of T (a suffix that is a
 * prefix of another sorts before it: libdivsufsort's divsufsort); isa[i] is the row of suffix i, isa[sa[r]] = r.  The sort is
 * bce_hip_divbwt's -- K1 on the n + 1 rotations of T$ with a unique smallest sentinel, which orders them as suffixes -- with its
 * order kept: one pass copies rows 1 .. n out and, where isa_out is not NULL, the rank array the sort maintains as the inverse
 * (8 n bytes read and written a side).  Nothing is cached: every call sorts.
 * State: as bce_hip_divbwt, the context's compression state is DROPPED (planes, suffix array and loaded input of an earlier load are
 * gone: the index queries answer BCE_HIP_E_STATE afterwards, a later load and compression give the archive of a fresh context).
 * Device memory held: what bce_hip_divbwt holds, plus 4 n bytes per output staged for a call with host buffers.
 * A null ctx, in or sa_out, n == 0, n >= 2^31 - 1: BCE_HIP_E_ARG before any device call; isa_out may be NULL. */
int bce_hip_suffix_array(bce_hip_ctx *ctx, const uint8_t *in, uint32_t n, uint32_t *sa_out, uint32_t *isa_out /* may be NULL */);
/* The same with the bytes and both outputs in device memory of the context's device.  d_in is copied into the context's text
 * buffer; the outputs are 4-byte aligned, n words each, and may not overlap d_in or each other.  Only the status comes back.
 * Stream rule: as bce_hip_count_device. */
int bce_hip_suffix_array_device(bce_hip_ctx *ctx, const void *d_in, uint32_t n, void *d_sa, void *d_isa /* may be NULL */);
/* Is sa[0, n) -- ANY n words, read as unsigned -- the suffix array of in[0, n), 0 < n < 2^31?  Linear work, on the device, in three
 * stages; the first stage that finds something decides, so *reason and *bad are a function of the two inputs alone:
 *   BCE_HIP_SUFCHECK_RANGE    *bad = the smallest row i with sa[i] >= n;
 *   BCE_HIP_SUFCHECK_MISSING  every entry is in range, and *bad = the smallest text position that no row names (an entry that
 *                             stands twice leaves one);
 *   BCE_HIP_SUFCHECK_ORDER    the array is a permutation, and *bad = the smallest row i >= 1 that breaks the rule: with a = sa[i - 1]
 *                             and b = sa[i], either in[a] < in[b], or in[a] == in[b] and a + 1 == n, or in[a] == in[b], b + 1 < n and
 *                             suffix a + 1 stands in a row above suffix b + 1's.  A permutation keeps the rule on every row
 *                             exactly when it is sorted (Burkhardt and Karkkainen's inductive check);
 *   BCE_HIP_SUFCHECK_OK       none of these: *bad = UINT64_MAX.  n == 1 is sound when sa[0] == 0.
 * An array that is not sorted is NOT an error: the call returns BCE_HIP_OK and the verdict is in *reason and *bad (host pointers,
 * both required).  Block reductions without atomics; twelve bytes come back.  Device memory held: 4 n bytes for the inverse the
 * second stage builds, 12 bytes per 2048 rows, plus the 5 n bytes of a call with host buffers, staged.
 * State: valid in ANY state of the context, between the stages of a compression included: only buffers of the checker's own are
 * written and nothing a stage keeps is read, so an encode after a check gives the archive of a fresh context.
 * A null ctx, in, sa, bad or reason, n == 0, n >= 2^31: BCE_HIP_E_ARG before any device call, the outputs untouched. */
#define BCE_HIP_SUFCHECK_OK 0u
#define BCE_HIP_SUFCHECK_RANGE 1u
#define BCE_HIP_SUFCHECK_MISSING 2u
#define BCE_HIP_SUFCHECK_ORDER 3u
int bce_hip_sufcheck(bce_hip_ctx *ctx, const uint8_t *in, const uint32_t *sa, uint32_t n, uint64_t *bad, uint32_t *reason);
/* The same with the bytes and the array (4-byte aligned) in device memory of the context's device; bad and reason stay host
 * pointers.  Neither array is written.  Stream rule: as bce_hip_count_device. */
int bce_hip_sufcheck_device(bce_hip_ctx *ctx, const void *d_in, const void *d_sa, uint32_t n, uint64_t *bad, uint32_t *reason);

/* ---- test hooks: the device primitives every stage rests on, alone (tests/test_gpu_sort.py, tests/test_gpu_compare.py) ----
 * Stream rule of bce_hip_crc32_device for all three: the work runs on the context's stream and is complete on return; the caller's
 * memory (device memory of the context's device) must be ready when the call is made.  Valid in any state of the context, between
 * the stages of a compression and between two bce_hip_model_flush calls included: they write the caller's arrays, the sorter's
 * histograms and buffers that only these hooks use, nothing that a stage keeps. */
/* Test hook: radix_sort.hip's radix_sort_pairs -- the sort K1, the enumeration's tail, K4 and the decoder call -- on n (u32 key,
 * u32 value) pairs of the caller's: stable LSD sort on key bits [first_bit, first_bit + bits), in place (the context holds the
 * other halves of the ping-pong and copies the result back when it lands there); the key bits outside the window travel with their
 * pair.  max_digit_bits = the widest digit of a pass, 1..10 (anything else counts as 8), as the callers pass it.
 * first_bit + bits > 32, or n > 0 with a null pointer: BCE_HIP_E_ARG; n <= 1 or bits == 0: success, nothing touched. */
int bce_hip_sort_pairs_device(bce_hip_ctx *ctx, void *d_key, void *d_val, uint32_t n, uint32_t first_bit, uint32_t bits,
                              uint32_t max_digit_bits);
/* Test hook: the same for radix_sort_wide (K1's first sort): 64-bit keys in two u32 arrays (hi:lo), sorted on key bits [0, bits).
 * bits > 64, or n > 0 with a null pointer: BCE_HIP_E_ARG. */
int bce_hip_sort_wide_device(bce_hip_ctx *ctx, void *d_lo, void *d_hi, void *d_val, uint32_t n, uint32_t bits,
                             uint32_t max_digit_bits);
/* Test hook: kd_compare.hip, the comparison behind bce_hip_verify_device / _host, on two buffers of the caller's, any alignment
 * each: *first_diff = the smallest i < n with a[i] != b[i], UINT64_MAX when there is none (n == 0 included: pointers ignored).
 * Reads [0, n) of both and nothing else.  A null ctx or first_diff, n > 0 with a null buffer: BCE_HIP_E_ARG. */
int bce_hip_compare_device(bce_hip_ctx *ctx, const void *d_a, const void *d_b, size_t n, uint64_t *first_diff);

/* ---- test hooks: the back end of the GPU decoder alone (kd_decode.hip; tests/test_gpu_unbwt.py) ----
 * The two stages a decode runs after its last round, on arrays of the caller's in device memory of the context's device, with the
 * launches and launch geometry of a decode (the decoder calls the same two functions).  Stream rule of the hooks above.  Unlike
 * them these two are a decode as far as the context goes: whatever compression state it holds is dropped (as by any decode) and
 * the decoder's scratch buffers are written, so they are valid wherever a decode is, and an encode or decode that follows finds
 * the context as after a decode.  n == 0, n >= 2^31 - 1 or a null ctx / required pointer: BCE_HIP_E_ARG, before any device work. */
/* Test hook: boundary ranks -> plane words and word ranks -> rank granules -> BWT bytes (fill_*_kernel, gran_from_words_kernel,
 * access_kernel).  d_R: u32 [8][n + 1], R[p][i] = the ones of plane p in front of position i where known, 0xFFFFFFFF where not.
 * R[p][0] (which must be 0) and R[p][n] must be known -- anything else, or R[p][n] > n: BCE_HIP_E_ARG, read from the device before
 * anything is launched -- and between two neighbouring known indices a plane must be constant.  The planes' zero counts are taken
 * from the array as the decoder takes them from the archive's header, zeros[p] = n - R[p][n].  A gap that is neither all zeros nor
 * all ones, or a rank that decreases: BCE_HIP_E_INTERNAL, "decode: a mixed gap was never split", with no output written.
 * d_bwt_out: the n bytes.  d_words_out, d_rankw_out (each may be NULL): u32 [8][W], W = (n + 31) / 32 + 3 -- the plane bits LSB
 * first and the rank at each word's first position, zero in the words wholly past n (the rank of the word that starts AT n
 * is kept). */
int bce_hip_planes_from_ranks_device(bce_hip_ctx *ctx, const void *d_R, uint32_t n, void *d_bwt_out, void *d_words_out,
                                     void *d_rankw_out);
/* Test hook: the inverse BWT (lf_keys_kernel, one 8-bit radix pass, lf_scatter_kernel, the concurrent walkers of lf_walk, and
 * expand_cycle_kernel for a periodic text) of the n bytes at d_bwt into d_out (any alignment; it may not overlap d_bwt): text
 * position i lands at d_out[(i + offset) % n].  `offset` is reduced modulo n here, as the decoder reduces the archive's.
 * *cycle_len (may be NULL): the length of the LF cycle through row 0 -- n for a primitive text, the period's share for a periodic
 * one; *walkers (may be NULL): the walkers launched, ((n - 1) >> sh) + 1.  Both are set on BCE_HIP_E_INTERNAL as well: "decode: LF
 * cycle of length L in n rows" -- L does not divide n, or is 0 (a walker's segment met twice) -- and then nothing of d_out is
 * written. */
int bce_hip_unbwt_device(bce_hip_ctx *ctx, const void *d_bwt, uint32_t n, uint32_t offset, void *d_out, uint64_t *cycle_len,
                         uint32_t *walkers);

/* ---- test hooks: the block scans of the index queries alone (kd_lcp.hip, kd_match.hip; tests/test_gpu_index_scans.py) ----
 * The reductions behind bce_hip_kgrams, bce_hip_longest_repeat and bce_hip_coverage on arrays of the caller's in device memory of
 * the context's device, with the launches and launch geometry of the real calls (which run the same functions): 2048-element
 * blocks, one workgroup that walks the blocks' results 256 at a time, the blocks again.  An input need not come from any text, so
 * a class or a match can be put across any block and any pass of the walk.  Stream rule of the hooks above.  Valid in any state of
 * the context, as the sort hooks: they write buffers of the features' own and nothing that a stage keeps. */
/* Test hook: kd_kgrams and, where repeat3 != NULL, kd_longest_repeat on the n words at d_lcp read as an LCP array (d_lcp[0] must
 * be 0) with the n words at d_sa as the suffix array.  Both arrays 4-byte aligned, nothing more: the LCP words are copied, device to
 * device, into the context's own array first, which keeps the 32-byte alignment the reductions' loads rest on -- as the real path
 * does, whose array is always the context's.  out[i] = the record of ks[i], i < nk <= BCE_HIP_KGRAMS_MAX (ks and out host arrays;
 * max_pos = d_sa[the first row of the lowest-row class of the largest size]); repeat3[0] = the largest word, repeat3[1], [2] =
 * d_sa[r - 1], d_sa[r] of the lowest row r that reaches it, 0xFFFFFFFF twice where it is 0.  Writes only the feature's rep_*
 * buffers.  A null ctx, d_lcp or d_sa, n == 0, n >= 2^31, nk > BCE_HIP_KGRAMS_MAX, nk > 0 with a null ks or out: BCE_HIP_E_ARG
 * before any device call. */
int bce_hip_lcp_reduce_device(bce_hip_ctx *ctx, const void *d_lcp, uint32_t n, const void *d_sa, const uint32_t *ks, uint32_t nk,
                              bce_hip_kgram *out, uint32_t repeat3[3]);
/* Test hook: the selection of bce_hip_top_kgrams (kd_top_kgrams) on the n words at d_lcp read as an LCP array (d_lcp[0] must be 0)
 * with the n words at d_sa as the suffix array, copied and aligned as above.  No bytes are gathered.  out: a HOST array with room
 * for limit entries (pos = d_sa[row]); found, distinct (may be NULL) and size_hist (may be NULL) as in the real call.  Writes only
 * rep_lcp and the feature's top_* buffers.  A null ctx, d_lcp, d_sa, out or found, n == 0, n >= 2^31, k above
 * BCE_HIP_MATCH_MAX_LEN, a limit outside 1 .. BCE_HIP_TOP_MAX: BCE_HIP_E_ARG before any device call. */
int bce_hip_top_classes_of_lcp_device(bce_hip_ctx *ctx, const void *d_lcp, uint32_t n, const void *d_sa, uint32_t k, uint32_t limit,
                                      bce_hip_top_kgram *out, uint32_t *found, uint64_t *distinct, uint64_t size_hist[32]);
/* Test hook: the launches of bce_hip_maximal_repeats behind its LCP pass, with the same geometry, on arrays of the caller's: the n
 * words at d_lcp read as the LCP array (d_lcp[0] must be 0; words of 0xFFFFFFFF name no interval; copied and aligned as above), the n
 * words at d_sa as the suffix array (pos = d_sa[row]) and the n bytes at d_bw in place of the text's preceding bytes.  No bytes are
 * gathered.  out: a HOST array with room for limit entries.  Valid in any state of the context; writes only rep_lcp, slf_tree,
 * slf_top and the feature's mxr_* buffers.  A null ctx, d_lcp, d_sa, d_bw, out or info, n == 0, n >= 2^31, 1 <= min_len <= max_len <=
 * BCE_HIP_MATCH_MAX_LEN violated, an unknown order, a limit outside 1 .. BCE_HIP_TOP_MAX: BCE_HIP_E_ARG before any device call. */
int bce_hip_maxrep_of_arrays_device(bce_hip_ctx *ctx, const void *d_lcp, uint32_t n, const void *d_sa, const void *d_bw, uint32_t min_len,
                                    uint32_t max_len, uint32_t order, uint32_t limit, bce_hip_maxrep *out, bce_hip_maxrep_info *info);
/* Test hook: kd_coverage, the reduction of bce_hip_coverage, on q lengths of the caller's (u32, 4-byte aligned) with
 * d_len[i] <= i + 1 (a match does not start in front of the query): *covered = the j < q for which some i >= j has
 * d_len[i] >= min_len and i - d_len[i] + 1 <= j.  Writes only mat_res and mat_bsum.  q == 0: *covered = 0, d_len ignored.  A null
 * ctx or covered, q >= 2^31, a min_len outside 1 .. BCE_HIP_MATCH_MAX_LEN, q > 0 with a null d_len: BCE_HIP_E_ARG before any device
 * call. */
int bce_hip_coverage_of_lengths_device(bce_hip_ctx *ctx, const void *d_len, uint64_t q, uint32_t min_len, uint64_t *covered);

/* ---- statistics of the last bce_hip_encode / bce_hip_compress ------------------------------------ */
typedef struct bce_hip_stats {
  uint64_t n;            /* input bytes */
  uint64_t nodes;        /* nodes visited (= 8n-8 on primitive inputs) */
  uint64_t symbols;      /* coded symbols (adaptive calls, bce.cpp:1302) */
  uint32_t rounds;       /* rounds of BCE::code */
  uint32_t sort_rounds;  /* prefix-doubling rounds of K1 */
  uint32_t flushes;      /* K4 model flushes */
  uint32_t spine_levels; /* byte levels of the enumeration's tail done by spine bursts (k3_dfs.hip) */
  /* t_load, t_bwt, t_planes, t_total: host wall seconds.  t_enum, t_model: GPU seconds (HIP events) of K3 and of
   * K4 + device-to-host copies.  t_coder: host seconds spent waiting for the coder threads (the part of the range
   * coding that nothing hides).  The last three overlap, so they do not add up to t_total. */
  double t_load, t_bwt, t_planes, t_enum, t_model, t_coder, t_total;
  double k3_ms, k3_launches;   /* HIP-event time and launch count of the interval-count kernels */
  double t_coder_busy;         /* busiest host coder thread (t_coder is only the part not hidden behind GPU work) */
  double list_grows;           /* times a round did not fit the node lists and they were doubled (k3_grow_lists) */
  double list_nodes;           /* nodes per list at the end (the larger of the two parities) */
  double split_rounds;         /* rounds whose symbols did not fit one model flush and were run plane group by plane group */
  /* since the context was created (not reset by a load): */
  double reg_maps;             /* host mappings registered with the runtime (flush slots, the decoder's boundary ranks) */
  double reg_unmaps;           /* ... and given back (after waiting for the work that touches them) */
  double dec_restarts;         /* GPU-assisted decodes started again with larger node lists (kd_decode.hip; stays 0: the lists grow in place) */
  double t_model_kernels;      /* of t_model: GPU seconds of K4's kernels alone (sort, window, long, emit), without the device-to-host copies */
  /* since the context was created (not reset by a load), like dec_restarts: */
  double dec_list_grows;       /* GPU-assisted decodes: a node list replaced by a larger one in the middle of a round (kd_decode.hip) */
  double dec_split_rounds;     /* GPU-assisted decodes: rounds with more nodes than the query budget, run plane group by plane group */
} bce_hip_stats;
int bce_hip_get_stats(const bce_hip_ctx *ctx, bce_hip_stats *out);

/* ---- synthetic inputs (SURVEY.md section 8c generators; host side, for benchmarks and tests) ------- */
void bce_hip_synth_text(uint64_t seed, uint8_t *out, size_t n);
void bce_hip_synth_rand(uint64_t seed, uint8_t *out, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* BCE_HIP_H */
