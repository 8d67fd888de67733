// main.cpp -- the `bce` command line, mirroring the reference's main() (bce.cpp:1376-1484):
//   bce -c archive.bce file [config.bcc]    compress on the MI355X through libbcehip.so
//   bce -t file archive.bce                 (extension) decode on the GPU and compare with "file" there; writes nothing
//   bce -CN archive.bcem file [config.bcc]  (extension) as -cN, N = 1..64, with the CRC-32 of every block's text in the container
//   bce -t archive.bcem                     (extension) decode such a container on the GPU and test it against its own CRC-32s
//   bce -g PATTERN file                     (extension) how often the bytes of PATTERN occur in "file", counted on the GPU from its BWT planes
//   bce -gd PATTERN archive                 (extension) the same in what an archive or container holds
//   bce -gl PATTERN file, -gld PATTERN archive   (extension) where they occur: the byte offsets, gathered on the GPU from K1's suffix array
//   bce -gn K PATTERN file, -gnd K PATTERN archive   (extension) how often something occurs that differs from PATTERN in at most K (0..2) bytes, per distance
//   bce -gnl K PATTERN file, -gnld K PATTERN archive (extension) where: the byte offsets, each with its distance
//   bce -gw K PATTERN file, -gwd K PATTERN archive   (extension) how often something occurs within K (0..2) edits of PATTERN -- substitutions, insertions, deletions -- per distance
//   bce -gwl K PATTERN file, -gwld K PATTERN archive (extension) where: the byte offsets, each with the length and the distance of its best alignment
//   bce -gm MINLEN file query_file, -gmd MINLEN archive query_file   (extension) how much of a second file lies in strings of MINLEN bytes or more that occur in the first
//   bce -gr MINLEN file query_file out.bcd, -grd ... archive ...   (extension) writes query_file as a delta against the first: copies out of it plus the new bytes
//   bce -ga file in.bcd out_file, -gad archive in.bcd out_file     (extension) rebuilds a file from the first and a delta, both sides checked by CRC-32
//   bce -gk K file, -gkd K archive          (extension) the k-grams of the circular text for k = 0..K: how many, how many occur once, the most frequent, H_k; the longest repeat
//   bce -gp ORDER MINLEN N file, -gpd ..   (extension) the N heaviest maximal repeats of MINLEN bytes or more: length, count, one position and the bytes
//   bce -gf K N file, -gfd K N archive      (extension) the N most frequent K-grams of the circular text: count, one position and the bytes of each
//   bce -gz MINLEN file, -gzd MINLEN archive   (extension) the text as copies of its own earlier bytes: the greedy LZ77 factorisation, counted on the GPU
//   bce -gs file out.sa, -gsd archive out.sa   (extension) the suffix array of the text, sorted on the GPU, as native 32-bit words
//   bce -gsc file in.sa                        (extension) checks such a file against the text, on the GPU
// Banner, usage text, summary line, argument detection and exit codes follow the reference
// (banner :1377-1379, -c :1403-1427, -d :1428-1472, usage :1473-1483).  -d uses the GPU-assisted decoder (kd_decode.hip), -ds the host decoder (decoder.cpp);
// -s runs the enumeration on the GPU in scan mode and the ScanCoder optimisation on the host (scan_coder.cpp).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <chrono>
#include <exception>
#include <fstream>
#include <string>
#include <algorithm>
#include <atomic>
#include <thread>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/bce_hip.h"
#include "class_expr.h"
#include "top_step.h"

// "Coded: %u.%02u %%\r" as BCE::code prints it (bce.cpp:1354-1358); cleared at the end like :1372
static void progress(uint64_t done, uint64_t total, void *user) {
  uint64_t *prev = static_cast<uint64_t *>(user);
  const uint64_t cur = total ? done * 10000 / total : 0;
  if (cur > *prev) {
    printf("Coded: %llu.%02llu %%\r", (unsigned long long)(cur / 100), (unsigned long long)(cur % 100));
    fflush(stdout);
    *prev = cur;
  }
}
static void progress_end() { printf("                    \r"); }

// File::File (bce.cpp:842-856): the whole file in memory.  Read on a thread of its own while the main thread initialises the
// HIP runtime (bce_hip_create: ~0.1 s on this platform, the largest fixed cost of a one-shot run) -- plain read(2) into
// memory nobody has zeroed first (a std::vector's resize touches every page once more).
struct HostFile {
  uint8_t *p = nullptr;
  size_t n = 0;
  int status = -1;            // 0 ok, -1 not found / unreadable, -2 short read, -3 at or above the caller's size limit (nothing read)
  ~HostFile() { free(p); }
  const uint8_t *data() const { return p; }
  size_t size() const { return n; }
};
static void read_whole_file(const char *path, HostFile *f, size_t limit) {
  const int fd = open(path, O_RDONLY | O_CLOEXEC);
  if (fd < 0) return;
  struct stat st;
  if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode) || st.st_size < 0) { close(fd); return; }
  const size_t n = (size_t)st.st_size;
  if (limit && n >= limit) { close(fd); f->n = n; f->status = -3; return; }   // too large for the caller: not read at all
  f->p = static_cast<uint8_t *>(malloc(n ? n : 1));
  if (!f->p) { close(fd); return; }
  size_t got = 0;
  while (got < n) {
    const ssize_t r = read(fd, f->p + got, n - got);
    if (r <= 0) break;
    got += (size_t)r;
  }
  close(fd);
  f->n = got;
  f->status = got == n ? 0 : -2;
}

// n < 2^31: saidx_t / the 31-bit getv of the header (bce.cpp:173,374,901)
static const size_t kMaxInput = (size_t)0x80000000ull;

// Writes the whole output and says whether it arrived: a short or failed write (ENOSPC, EIO) must not end in the success
// line and exit code 0 -- after fast_exit nothing later could report it.
static bool write_file(const char *path, const void *p, size_t bytes) {
  std::ofstream f(std::string(path), std::ios::binary | std::ios::trunc);
  if (!f) return false;
  f.write(static_cast<const char *>(p), (std::streamsize)bytes);
  f.close();
  return f.good();
}

// The output is on disk and stdout is flushed: leave without the tear-down of 20 GB of device buffers, 400 MB of pinned
// memory and the runtime's own exit handlers (0.1-0.25 s that a user of a one-shot tool would wait for nothing; the kernel
// reclaims everything).  BCE_CLI_CLEAN_EXIT=1 takes the long way (leak checkers).
static void fast_exit(int code) {
  fflush(stdout);
  fflush(stderr);
  if (!getenv("BCE_CLI_CLEAN_EXIT")) _exit(code);
}

// ---- multi-block container (an extension; the reference has one block per archive, bce.cpp:1151-1157) ----
// b"BCEM" | u32 version = 1 | u32 nblocks | nblocks x (u64 raw_bytes, u64 archive_bytes) | the archives.  Every
// embedded archive is exactly what `bce -c` writes for that block alone.  Same layout as bce_amd/container.py
// (the 8-GPU path of bench.py gathers its blocks into it).  A plain archive cannot start with "BCEM": that would
// be a header of 0x4342 words.
// Version 2 (`bce -CN`): the same with table entries of (u64 raw_bytes, u64 archive_bytes, u32 CRC-32 of the block's text,
// u32 0) -- the archives are version 1's, and whoever decodes one can test it without the original.
static bool is_container(const HostFile &a) { return a.size() >= 12 && memcmp(a.data(), "BCEM", 4) == 0; }
static void put_u32(std::vector<uint8_t> &v, uint32_t x) { for (int i = 0; i < 4; ++i) v.push_back((uint8_t)(x >> (8 * i))); }
static void put_u64(std::vector<uint8_t> &v, uint64_t x) { for (int i = 0; i < 8; ++i) v.push_back((uint8_t)(x >> (8 * i))); }
static uint64_t get_le(const uint8_t *p, int bytes) { uint64_t x = 0; for (int i = 0; i < bytes; ++i) x |= (uint64_t)p[i] << (8 * i); return x; }
// the table of a container that archive_blocks has accepted: version, entry b's raw size and (version 2) CRC-32
static uint32_t container_version(const HostFile &a) { return is_container(a) ? (uint32_t)get_le(a.data() + 4, 4) : 0; }
static size_t table_entry_bytes(uint32_t version) { return version == 2 ? 24 : 16; }
static uint64_t table_raw(const HostFile &a, size_t b) { return get_le(a.data() + 12 + b * table_entry_bytes(container_version(a)), 8); }
static uint32_t table_crc(const HostFile &a, size_t b) { return (uint32_t)get_le(a.data() + 12 + b * 24 + 16, 4); }

// (Weak references: this file is also linked, for the sanitizer run of `-ds` on hostile archives, into a CPU-only program beside
//  "no device" stand-ins for just the entry points the older modes call.  With libbcehip.so they resolve like any other.)
extern "C" int bce_hip_verify_host(bce_hip_ctx *ctx, const uint8_t *archive, size_t len, const uint8_t *original, size_t n,
                                   uint64_t *first_diff) __attribute__((weak));
extern "C" int bce_hip_input_crc32(bce_hip_ctx *ctx, uint32_t *crc) __attribute__((weak));
extern "C" int bce_hip_decode_crc32(bce_hip_ctx *ctx, const uint8_t *archive, size_t len, size_t *decoded, uint32_t *crc) __attribute__((weak));
extern "C" int bce_hip_decompress_device_crc32(bce_hip_ctx *ctx, const uint8_t *archive, size_t len, uint8_t *out, size_t cap,
                                               size_t *out_len, uint32_t *crc) __attribute__((weak));
extern "C" int bce_hip_estimate_host(bce_hip_ctx *ctx, const uint8_t *in, uint32_t n, uint64_t plane_cost_q24[8], uint64_t plane_steps[8],
                                     size_t *archive_bytes) __attribute__((weak));

extern "C" int bce_hip_count(bce_hip_ctx *ctx, const uint8_t *patterns, const uint64_t *offsets, uint32_t npat, uint64_t *counts) __attribute__((weak));
extern "C" int bce_hip_locate(bce_hip_ctx *ctx, const uint8_t *patterns, const uint64_t *offsets, uint32_t npat, uint32_t flags, uint64_t *hit_offsets,
                              uint32_t *positions, uint64_t cap, uint64_t *total) __attribute__((weak));
extern "C" int bce_hip_count_near(bce_hip_ctx *ctx, const uint8_t *patterns, const uint64_t *offsets, uint32_t npat, uint32_t k, uint64_t *counts) __attribute__((weak));
extern "C" int bce_hip_locate_near(bce_hip_ctx *ctx, const uint8_t *patterns, const uint64_t *offsets, uint32_t npat, uint32_t k, uint32_t flags,
                                   uint64_t *hit_offsets, uint32_t *positions, uint8_t *dists, uint64_t cap, uint64_t *total) __attribute__((weak));
extern "C" int bce_hip_count_edit(bce_hip_ctx *ctx, const uint8_t *patterns, const uint64_t *offsets, uint32_t npat, uint32_t k, uint32_t flags,
                                  uint64_t *counts) __attribute__((weak));
extern "C" int bce_hip_locate_edit(bce_hip_ctx *ctx, const uint8_t *patterns, const uint64_t *offsets, uint32_t npat, uint32_t k, uint32_t flags,
                                   uint64_t *hit_offsets, uint32_t *positions, uint16_t *lens, uint8_t *dists, uint64_t cap, uint64_t *total) __attribute__((weak));
extern "C" int bce_hip_count_classes(bce_hip_ctx *ctx, const uint32_t *masks, const uint64_t *offsets, uint32_t npat, uint32_t max_nodes, uint64_t *counts,
                                     uint64_t *work, uint32_t *status) __attribute__((weak));
extern "C" int bce_hip_locate_classes(bce_hip_ctx *ctx, const uint32_t *masks, const uint64_t *offsets, uint32_t npat, uint32_t max_nodes, uint32_t flags,
                                      uint64_t *hit_offsets, uint32_t *status, uint32_t *positions, uint64_t cap, uint64_t *total) __attribute__((weak));
extern "C" int bce_hip_coverage(bce_hip_ctx *ctx, const uint8_t *query, uint64_t q, uint32_t min_len, uint32_t flags, uint64_t *covered) __attribute__((weak));
extern "C" int bce_hip_kgrams(bce_hip_ctx *ctx, const uint32_t *ks, uint32_t nk, bce_hip_kgram *out) __attribute__((weak));
extern "C" int bce_hip_longest_repeat(bce_hip_ctx *ctx, uint32_t max_len, uint32_t *len, uint32_t *pos_a, uint32_t *pos_b) __attribute__((weak));
extern "C" int bce_hip_top_kgrams(bce_hip_ctx *ctx, uint32_t k, uint32_t limit, bce_hip_top_kgram *out, uint8_t *bytes, uint64_t bytes_cap,
                                  uint32_t *found, uint64_t *distinct, uint64_t size_hist[32]) __attribute__((weak));
extern "C" int bce_hip_maximal_repeats(bce_hip_ctx *ctx, uint32_t min_len, uint32_t max_len, uint32_t order, uint32_t limit, bce_hip_maxrep *out,
                                       uint8_t *bytes, uint32_t bytes_per, uint64_t bytes_cap, bce_hip_maxrep_info *info) __attribute__((weak));
extern "C" int bce_hip_parse(bce_hip_ctx *ctx, const uint8_t *query, uint64_t q, uint32_t min_len, uint32_t max_len, bce_hip_op *ops, uint64_t ops_cap,
                             uint8_t *lits, uint64_t lits_cap, bce_hip_parse_info *info) __attribute__((weak));
extern "C" int bce_hip_patch(bce_hip_ctx *ctx, const bce_hip_op *ops, uint64_t nops, const uint8_t *lits, uint64_t nlits, uint8_t *out, uint64_t cap,
                             uint64_t *out_len) __attribute__((weak));
extern "C" int bce_hip_self_parse(bce_hip_ctx *ctx, uint32_t min_len, uint32_t max_len, bce_hip_op *ops, uint64_t ops_cap, uint8_t *lits,
                                  uint64_t lits_cap, bce_hip_parse_info *info) __attribute__((weak));
extern "C" int bce_hip_suffix_array(bce_hip_ctx *ctx, const uint8_t *in, uint32_t n, uint32_t *sa_out, uint32_t *isa_out) __attribute__((weak));
extern "C" int bce_hip_sufcheck(bce_hip_ctx *ctx, const uint8_t *in, const uint32_t *sa, uint32_t n, uint64_t *bad, uint32_t *reason) __attribute__((weak));

// `bce -cN`: N contiguous blocks over the GPUs of the node.  With more blocks than GPUs every device gets up to four
// gated contexts (bce_hip_set_gated), one host thread each: their GPU phases take turns while the coder threads of the
// context that has just left the GPU finish its block.  Blocks are handed out in order to whichever context is free.
// with_crc (`-CN`): a version-2 container -- every block's CRC-32 comes from the context that compressed it, which still holds
// the block's bytes on the device (bce_hip_input_crc32).
static int compress_blocks(const HostFile &data, uint32_t nblocks, const uint8_t *config, bool with_crc, std::vector<uint8_t> &out) {
  if (with_crc && !bce_hip_input_crc32) return BCE_HIP_E_DEVICE;
  std::vector<bce_hip_ctx *> ctx;
  int ndev = 0;
  for (int dev = 0; dev < 64; ++dev) {
    bce_hip_ctx *c = nullptr;
    if (bce_hip_create(&c, dev) != 0) break;
    ctx.push_back(c);
    ndev = dev + 1;
    if (ctx.size() >= nblocks) break;
  }
  if (ctx.empty()) return -3;
  const size_t per_dev = std::min<size_t>(4, (nblocks + (size_t)ndev - 1) / (size_t)ndev);
  for (size_t extra = 1; extra < per_dev; ++extra)
    for (int dev = 0; dev < ndev && ctx.size() < nblocks; ++dev) {
      bce_hip_ctx *c = nullptr;
      if (bce_hip_create(&c, dev) != 0) break;
      ctx.push_back(c);
    }
  for (size_t i = 0; i < ctx.size(); ++i) {
    if (config && bce_hip_set_config(ctx[i], config) != 0) {        // (validated by the caller already: cannot happen)
      printf("Config rejected: %s\n", bce_hip_last_error(ctx[i]));
      for (bce_hip_ctx *o : ctx) bce_hip_destroy(o);
      return -1;
    }
  }
  const size_t n = data.size(), base = n / nblocks, rem = n % nblocks;
  std::vector<std::vector<uint8_t>> arch(nblocks);
  std::vector<size_t> lo(nblocks + 1);
  for (uint32_t b = 0; b <= nblocks; ++b) lo[b] = b * base + (b < rem ? b : rem);
  std::vector<int> rcs(ctx.size(), 0);
  std::atomic<uint32_t> next_block{0};
  std::atomic<bool> failed{false};
  // A context that runs out of device memory (four contexts of a device and blocks of hundreds of MB: a context needs ~180
  // bytes per input byte) gives its memory back and leaves its block for later: what is left over is compressed at the end by
  // one context that has the device to itself.  Only a block that does not fit even then fails.
  std::mutex deferred_mu;
  std::vector<uint32_t> deferred;
  const char *test_nomem = getenv("BCE_CLI_TEST_NOMEM_BLOCK");      // (test hook: this block's first attempt "runs out of memory"; "all": every block's)
  const bool test_all = test_nomem && strcmp(test_nomem, "all") == 0;
  const long test_block = test_nomem && !test_all ? atol(test_nomem) : -1;
  std::vector<char> done(nblocks, 0);                               // block b's archive is in arch[b] (and, with_crc, its CRC-32 in crcs[b])
  std::vector<uint32_t> crcs(nblocks, 0);
  std::vector<std::thread> th;
  for (size_t d = 0; d < ctx.size(); ++d)
    th.emplace_back([&, d] {
      while (!failed.load()) {
        const uint32_t b = next_block.fetch_add(1);
        if (b >= nblocks) break;
        size_t alen = 0;
        int rc = (test_all || (long)b == test_block) ? BCE_HIP_E_NOMEM
                                         : bce_hip_compress(ctx[d], data.data() + lo[b], (uint32_t)(lo[b + 1] - lo[b]), nullptr, 0, &alen);
        if (rc == 0) { arch[b].resize(alen); rc = bce_hip_archive_copy(ctx[d], arch[b].data(), alen); }
        if (rc == 0 && with_crc) rc = bce_hip_input_crc32(ctx[d], &crcs[b]);
        if (rc == 0) done[b] = 1;
        if (rc == BCE_HIP_E_NOMEM) {
          { std::lock_guard<std::mutex> lk(deferred_mu); deferred.push_back(b); }
          bce_hip_destroy(ctx[d]);
          ctx[d] = nullptr;
          return;
        }
        if (rc) { rcs[d] = rc; failed.store(true); break; }
      }
      (void)bce_hip_set_gated(ctx[d], 1);                           // (gives the gate back if a failed stage left it held)
    });
  for (auto &t : th) t.join();
  int rc = 0;
  for (size_t d = 0; d < ctx.size(); ++d) {
    if (!ctx[d]) continue;
    if (rcs[d] && !rc) { rc = rcs[d]; printf("%s\n", bce_hip_last_error(ctx[d])); }
    bce_hip_destroy(ctx[d]);
  }
  // Every worker may have left that way (another tenant on the device, blocks too large for four contexts side by side):
  // the blocks nobody took are then in no list.  Whatever has no archive yet is compressed here, one block at a time.
  if (!rc) {
    deferred.clear();
    for (uint32_t b = 0; b < nblocks; ++b) if (!done[b]) deferred.push_back(b);
  }
  if (!rc && !deferred.empty()) {
    bce_hip_ctx *c = nullptr;
    rc = bce_hip_create(&c, 0);
    if (rc == 0 && config) rc = bce_hip_set_config(c, config);
    for (size_t i = 0; rc == 0 && i < deferred.size(); ++i) {
      const uint32_t b = deferred[i];
      size_t alen = 0;
      rc = bce_hip_compress(c, data.data() + lo[b], (uint32_t)(lo[b + 1] - lo[b]), nullptr, 0, &alen);
      if (rc == 0) { arch[b].resize(alen); rc = bce_hip_archive_copy(c, arch[b].data(), alen); }
      if (rc == 0 && with_crc) rc = bce_hip_input_crc32(c, &crcs[b]);
      if (rc == 0) done[b] = 1;                                     // (a block without its CRC is a block missing)
    }
    if (rc && c) printf("%s\n", bce_hip_last_error(c));
    if (c) bce_hip_destroy(c);
  }
  if (rc) return rc;
  for (uint32_t b = 0; b < nblocks; ++b)
    if (!done[b] || arch[b].empty()) return BCE_HIP_E_INTERNAL;     // a container never goes out with a block missing
  out.clear();
  out.insert(out.end(), {'B', 'C', 'E', 'M'});
  put_u32(out, with_crc ? 2 : 1);
  put_u32(out, nblocks);
  for (uint32_t b = 0; b < nblocks; ++b) {
    put_u64(out, lo[b + 1] - lo[b]);
    put_u64(out, arch[b].size());
    if (with_crc) { put_u32(out, crcs[b]); put_u32(out, 0); }
  }
  for (uint32_t b = 0; b < nblocks; ++b) out.insert(out.end(), arch[b].begin(), arch[b].end());
  return 0;
}

// The archives inside an archive file: (offset, length) of each -- one for a plain archive, the table's for a BCEM container.
// false: a container of an unknown version, one whose table does not fit the file, or (version 2) with a reserved word that is not 0.
static bool archive_blocks(const HostFile &adata, std::vector<std::pair<size_t, size_t>> &blocks) {
  if (!is_container(adata)) { blocks.emplace_back(0, adata.size()); return true; }
  const uint32_t ver = (uint32_t)get_le(adata.data() + 4, 4), nb = (uint32_t)get_le(adata.data() + 8, 4);
  const size_t entry = table_entry_bytes(ver);
  size_t pos = 12 + (size_t)nb * entry;
  if ((ver != 1 && ver != 2) || pos > adata.size()) return false;
  for (uint32_t b = 0; b < nb; ++b) {
    const size_t alen = (size_t)get_le(adata.data() + 12 + (size_t)b * entry + 8, 8);
    if (ver == 2 && get_le(adata.data() + 12 + (size_t)b * entry + 20, 4) != 0) return false;
    if (alen > adata.size() - pos) return false;
    blocks.emplace_back(pos, alen);
    pos += alen;
  }
  return true;
}

// exit status of `bce -t` when the archive decodes, but not to the file's bytes (every other failure keeps the status -d gives it)
static const int kExitDiffers = 1;

// `bce -t file archive.bce` (an extension): the archive is decoded on the GPU and compared THERE with the file, block by block for
// a container (bce_hip_verify_host: the decoded text never comes back to the host).  Nothing is written.
static int test_archive(const char *file_path, const char *archive_path) {
  auto start = std::chrono::high_resolution_clock::now();
  HostFile adata, data;
  std::thread areader(read_whole_file, archive_path, &adata, (size_t)0);
  std::thread freader(read_whole_file, file_path, &data, (size_t)0);
  bce_hip_ctx *ctx = nullptr;
  const int rc0 = bce_hip_create(&ctx, 0);
  areader.join();
  freader.join();
  struct Destroy { bce_hip_ctx *&c; ~Destroy() { if (c) bce_hip_destroy(c); } } destroy{ctx};
  if (adata.status == -1) { printf("Archive not found.\n"); return -1; }
  if (adata.status != 0 || adata.size() == 0) { printf("Could not read Archive.\n"); return -2; }
  if (data.status != 0) { printf("Error loading file\n"); return -1; }
  if (rc0 != 0 || !bce_hip_verify_host) { printf("No usable HIP device: %s\n", bce_hip_strerror(rc0 ? rc0 : BCE_HIP_E_DEVICE)); return -3; }
  std::vector<std::pair<size_t, size_t>> blocks;
  if (!archive_blocks(adata, blocks)) { printf("Could not read Archive.\n"); return -2; }
  // where each block's text begins in the whole file: from the blocks' own headers (a container's table must agree with them, as for -d)
  std::vector<uint64_t> at(blocks.size() + 1, 0);
  for (size_t b = 0; b < blocks.size(); ++b) {
    size_t hn = 0;
    const int hr = bce_hip_decompress(adata.data() + blocks[b].first, blocks[b].second, nullptr, 0, &hn);
    if (hr != 0 && blocks.size() == 1) { printf("Decompression failed: %s\n", bce_hip_strerror(hr)); return -4; }
    if (hr != 0 || (blocks.size() > 1 && (uint64_t)hn != table_raw(adata, b))) { printf("Could not read Archive.\n"); return -2; }
    at[b + 1] = at[b] + hn;
  }
  const uint64_t total = at.back(), fsize = data.size();
  uint64_t prog = 0;
  if (blocks.size() == 1) bce_hip_set_progress(ctx, progress, &prog);
  for (size_t b = 0; b < blocks.size(); ++b) {
    const uint64_t lo = std::min(at[b], fsize), len = std::min(at[b + 1] - at[b], fsize - lo);   // the file's slice for this block
    uint64_t fd = UINT64_MAX;
    const int rc = bce_hip_verify_host(ctx, adata.data() + blocks[b].first, blocks[b].second, data.data() + lo, (size_t)len, &fd);
    if (blocks.size() == 1) progress_end();
    if (rc != 0) {
      if (bce_hip_last_error(ctx)[0]) printf("%s\n", bce_hip_last_error(ctx));
      printf("Decompression failed: %s\n", bce_hip_strerror(rc));
      return -4;
    }
    if (fd == UINT64_MAX) continue;
    if (fd < len) printf("Archive differs from file at byte %llu\n", (unsigned long long)(at[b] + fd));
    else printf("Archive differs from file in size: the archive holds %llu B, the file %llu B (equal up to byte %llu)\n",
                (unsigned long long)total, (unsigned long long)fsize, (unsigned long long)fsize);
    fflush(stdout);
    return kExitDiffers;
  }
  if (fsize != total) {                                             // (a longer file: every block agreed with its slice)
    printf("Archive differs from file in size: the archive holds %llu B, the file %llu B (equal up to byte %llu)\n",
           (unsigned long long)total, (unsigned long long)fsize, (unsigned long long)total);
    return kExitDiffers;
  }
  std::chrono::duration<double> duration = std::chrono::high_resolution_clock::now() - start;
  printf("Archive OK: %zu B -> %llu B in %.1f s\n", adata.size(), (unsigned long long)total, duration.count());
  ctx = nullptr;                                                    // (left to fast_exit, like -d)
  fast_exit(0);
  return 0;
}

static void print_mismatch(size_t block, uint32_t table, uint32_t decoded) {
  printf("Checksum mismatch in block %zu: table %08X, decoded %08X\n", block, (unsigned)table, (unsigned)decoded);
}

// `bce -t archive.bcem` (an extension): a version-2 container tested against its own CRC-32s.  Every block is decoded on the GPU
// into the context's buffer and checksummed there (bce_hip_decode_crc32): no file is read or uploaded, nothing of the text comes
// back, nothing is written.  An archive without checksums gets its answer before any device is asked for.
static const int kExitNoChecksum = 2;
static int self_test_archive(const char *archive_path) {
  auto start = std::chrono::high_resolution_clock::now();
  HostFile adata;
  read_whole_file(archive_path, &adata, (size_t)0);
  if (adata.status == -1) { printf("Archive not found.\n"); return -1; }
  if (adata.status != 0 || adata.size() == 0) { printf("Could not read Archive.\n"); return -2; }
  if (container_version(adata) != 2) {
    if (is_container(adata) && container_version(adata) != 1) { printf("Could not read Archive.\n"); return -2; }
    printf("Archive carries no checksum: test it against the file (bce -t file archive)\n");
    return kExitNoChecksum;
  }
  std::vector<std::pair<size_t, size_t>> blocks;
  if (!archive_blocks(adata, blocks)) { printf("Could not read Archive.\n"); return -2; }
  uint64_t total = 0;
  for (size_t b = 0; b < blocks.size(); ++b) {                      // the table's sizes must be the blocks' own, as for -d
    size_t hn = 0;
    const uint64_t raw = table_raw(adata, b);
    if (bce_hip_decompress(adata.data() + blocks[b].first, blocks[b].second, nullptr, 0, &hn) != 0 || raw < 1 || raw >= 0x80000000ull || (uint64_t)hn != raw) {
      printf("Could not read Archive.\n");
      return -2;
    }
    total += raw;
  }
  bce_hip_ctx *ctx = nullptr;
  const int rc0 = bce_hip_create(&ctx, 0);
  struct Destroy { bce_hip_ctx *&c; ~Destroy() { if (c) bce_hip_destroy(c); } } destroy{ctx};
  if (rc0 != 0 || !bce_hip_decode_crc32) { printf("No usable HIP device: %s\n", bce_hip_strerror(rc0 ? rc0 : BCE_HIP_E_DEVICE)); return -3; }
  for (size_t b = 0; b < blocks.size(); ++b) {
    size_t n = 0;
    uint32_t crc = 0;
    int rc = bce_hip_decode_crc32(ctx, adata.data() + blocks[b].first, blocks[b].second, &n, &crc);
    if (rc == 0 && (uint64_t)n != table_raw(adata, b)) rc = BCE_HIP_E_INTERNAL;
    if (rc != 0) {
      if (bce_hip_last_error(ctx)[0]) printf("%s\n", bce_hip_last_error(ctx));
      printf("Decompression failed: %s\n", bce_hip_strerror(rc));
      return -4;
    }
    if (crc != table_crc(adata, b)) { print_mismatch(b, table_crc(adata, b), crc); fflush(stdout); return kExitDiffers; }
  }
  std::chrono::duration<double> duration = std::chrono::high_resolution_clock::now() - start;
  printf("Archive OK: %zu B -> %llu B in %.1f s\n", adata.size(), (unsigned long long)total, duration.count());
  ctx = nullptr;                                                    // (left to fast_exit, like -d)
  fast_exit(0);
  return 0;
}

// load_config, bce.cpp:626-641: the 288 bytes of `path` into cfgbuf and into the context -- or, with the reference's message, the
// defaults (cfgbuf left empty).
static void read_config(const char *path, bce_hip_ctx *ctx, std::vector<uint8_t> &cfgbuf) {
  std::ifstream cfg(path, std::ios::binary | std::ios::ate);
  std::streamoff size = cfg ? (std::streamoff)cfg.tellg() : -1;
  if (size != (std::streamoff)BCE_HIP_CONFIG_BYTES) {
    printf("Config not found or wrong size.\n");
  } else {
    cfgbuf.resize(BCE_HIP_CONFIG_BYTES);
    cfg.seekg(0, std::ios::beg);
    if (!cfg.read(reinterpret_cast<char *>(cfgbuf.data()), size)) { printf("Could not read Config.\n"); cfgbuf.clear(); }
    else if (bce_hip_set_config(ctx, cfgbuf.data()) != 0) { printf("Config rejected: %s\n", bce_hip_last_error(ctx)); cfgbuf.clear(); }
  }
}

// `bce -e file [config.bcc]` (extension): the size `bce -c` would write, from the model's code lengths summed on the GPU
// (bce_hip_estimate_host); the range coders do not run and nothing is written.
static int estimate_file(const char *file, const char *config) {
  HostFile data;
  std::thread reader(read_whole_file, file, &data, kMaxInput);      // as -c: beside the runtime's start-up
  bce_hip_ctx *ctx = nullptr;
  const int rc0 = bce_hip_create(&ctx, 0);
  reader.join();
  if (rc0 != 0 || !bce_hip_estimate_host) {
    printf("No usable HIP device: %s\n", bce_hip_strerror(rc0 ? rc0 : BCE_HIP_E_DEVICE));
    if (ctx) bce_hip_destroy(ctx);
    return -3;
  }
  std::vector<uint8_t> cfgbuf;
  if (config) read_config(config, ctx, cfgbuf);
  if (data.status != 0 || data.size() == 0 || data.size() >= kMaxInput) { printf("Error loading file\n"); bce_hip_destroy(ctx); return -1; }
  uint64_t cost[8], steps[8], prog = 0;
  size_t bytes = 0;
  bce_hip_set_progress(ctx, progress, &prog);
  const int rc = bce_hip_estimate_host(ctx, data.data(), (uint32_t)data.size(), cost, steps, &bytes);
  progress_end();
  if (rc != 0) { printf("Estimate failed: %s (%s)\n", bce_hip_strerror(rc), bce_hip_last_error(ctx)); bce_hip_destroy(ctx); return -4; }
  printf("Estimated size: %zu B (ratio %.4f)\n", bytes, (double)bytes / (double)data.size());
  printf("Plane bits:");
  for (int p = 0; p < 8; ++p) printf(" %.1f", (double)cost[p] / 16777216.0);
  printf("\n");
  fast_exit(0);
  bce_hip_destroy(ctx);
  return 0;
}

// `bce -g PATTERN file` / `bce -gd PATTERN archive` (extensions): how often the literal bytes of PATTERN occur in the file, or in
// what the archive (a plain one, or a BCEM container of either version) decodes to -- overlapping matches counted, as a scan of the
// text would find them.  K1 and K2 index the text on the GPU and backward search on the planes counts the matches in the circular
// text (bce_hip_count); those that run across the end of the text are found here, in its last and first m - 1 bytes, and come off.
// An archive's blocks are decoded by the GPU-assisted decoder, one after the other, a version-2 container's against their CRC-32s.
// `-gl` / `-gld` (locate): the same files, answers and exit codes; the matches' byte offsets, one per line, ascending, come before
// the count line.  They are the linear hits of bce_hip_locate: gathered from K1's suffix array and filtered on the GPU.
// `-gm MINLEN file query_file` / `-gmd MINLEN archive query_file` (coverage): the file or archive is read, judged, decoded and indexed
// in the same way; query_file is a plain file, judged with the words of -g's.  One line: how many of its bytes lie in strings of
// MINLEN bytes or more that occur in the indexed text (bce_hip_coverage, linear matches: searched and reduced on the GPU).
// `-gk K file` / `-gkd K archive` (k-grams): the file or archive is read, judged, decoded and indexed in the same way.  For k = 0..K
// one line: the distinct k-grams of the CIRCULAR text, those that occur once, the occurrences of the most frequent one and the order-k
// empirical entropy H_k = max(0, S_k - S_(k+1)) / (n 2^24) from the integer sums of bce_hip_kgrams; then the longest repeat
// (bce_hip_longest_repeat at the bound 4096) and the text's size.  Two LCP passes, bounded by K + 1 and by 4096: nothing is cached.
static uint64_t seam_matches(const uint8_t *t, size_t n, const uint8_t *pat, size_t m) {
  std::vector<uint8_t> seam(t + n - (m - 1), t + n);
  seam.insert(seam.end(), t, t + (m - 1));
  uint64_t found = 0;
  for (size_t s = 0; s + m <= seam.size(); ++s) found += memcmp(seam.data() + s, pat, m) == 0;
  return found;
}
constexpr uint32_t kMaxKgramOrder = 32;                            // -gk / -gkd: the largest K
// `-gf K N file` / `-gfd K N archive` (most frequent): the file or archive is read, judged, decoded and indexed in the same way.  A head
// line, then the first N classes of bce_hip_top_kgrams for K, most frequent first and among equal counts in the order of the bytes:
// count, the position of one occurrence, the K bytes (top_step.h: top_escape); then the distinct K-grams and the text's size.
constexpr uint32_t kMaxTopLen = 256, kMaxTopCount = 65536;          // -gf / -gfd: the largest K and N
// `-gr MINLEN file query_file out.bcd` / `-grd` (delta): the file or archive is read, judged, decoded and indexed in the same way,
// query_file judged as -gm's; the query is parsed on the GPU (bce_hip_parse at the bounds MINLEN and max(256, MINLEN)) and written
// as a delta file.  `-ga file in.bcd out_file` / `-gad` (apply): in.bcd is read and judged as -d judges an archive, before the
// device is missed; the base's size and CRC-32 (taken on the GPU) are checked before the patch, the result's after it, and a
// mismatch on either side ends with kExitDiffers and writes nothing.
// The delta file, little-endian: "BCED" | u32 version = 1 | u64 n | u32 crc32(base) | u64 q | u32 crc32(result) | u32 min_len |
// u32 max_len | u64 nops | u64 nlits | nops x (u32 len, u32 src) | nlits bytes   (bce_amd/container.py: pack_delta / unpack_delta)
constexpr size_t kDeltaHeader = 56;
constexpr uint32_t kDeltaMaxLen = 256;                             // the length bound of -gr's search, where MINLEN is not above it
struct DeltaHeader { uint64_t n, q, nops, nlits; uint32_t base_crc, crc, min_len, max_len; };
template <class T> static T le_at(const uint8_t *p) { T v; memcpy(&v, p, sizeof v); return v; }
// the magic, the version, sizes that add up to the file's length without overflow, a base and a result below 2^31 bytes
static bool read_delta_header(const uint8_t *p, size_t len, DeltaHeader &h) {
  if (len < kDeltaHeader || memcmp(p, "BCED", 4) != 0 || le_at<uint32_t>(p + 4) != 1) return false;
  h.n = le_at<uint64_t>(p + 8); h.base_crc = le_at<uint32_t>(p + 16); h.q = le_at<uint64_t>(p + 20); h.crc = le_at<uint32_t>(p + 28);
  h.min_len = le_at<uint32_t>(p + 32); h.max_len = le_at<uint32_t>(p + 36); h.nops = le_at<uint64_t>(p + 40); h.nlits = le_at<uint64_t>(p + 48);
  const uint64_t room = len - kDeltaHeader;
  if (h.nops > room / 8 || h.nlits != room - h.nops * 8) return false;
  return h.q < kMaxInput && h.n < kMaxInput && (h.n != 0 || h.nops == 0);
}
static void write_delta_header(uint8_t *p, const DeltaHeader &h) {
  const uint32_t ver = 1;
  memcpy(p, "BCED", 4); memcpy(p + 4, &ver, 4); memcpy(p + 8, &h.n, 8); memcpy(p + 16, &h.base_crc, 4); memcpy(p + 20, &h.q, 8);
  memcpy(p + 28, &h.crc, 4); memcpy(p + 32, &h.min_len, 4); memcpy(p + 36, &h.max_len, 4); memcpy(p + 40, &h.nops, 8); memcpy(p + 48, &h.nlits, 8);
}
// ---- the front of all twenty-three index commands ----
// The indexed file (or archive) and the command's second file are read beside the runtime's start-up and judged in this order: the
// file or archive, the second file, the device; an archive's blocks are then decoded into one text.  Owns the context: an error
// path destroys it, index_done() leaves it to fast_exit.
enum SecondFile { kNoSecond, kSecondQuery, kSecondDelta, kSecondArray };
struct IndexInput {
  HostFile file, second;                                              // second: the query of -gm / -gr, the delta of -ga, the array of -gsc
  bool one_text = false;                                              // -gsd: a container is refused, its blocks are separate texts
  DeltaHeader dh{};                                                   // of the delta
  std::vector<uint8_t> decoded;
  bce_hip_ctx *ctx = nullptr;
  const uint8_t *text = nullptr;
  size_t n = 0;
  ~IndexInput() { if (ctx) bce_hip_destroy(ctx); }
};
// 0, or the command's exit code with its line printed.  have_api: the library has the entry points the command calls.
static int index_open(IndexInput &in, const char *path, bool in_archive, const char *second_path, SecondFile second, bool have_api) {
  HostFile &file = in.file, &query = in.second;
  std::thread reader(read_whole_file, path, &file, in_archive ? (size_t)0 : kMaxInput);   // beside the runtime's start-up
  std::thread query_reader;
  if (second != kNoSecond) query_reader = std::thread(read_whole_file, second_path, &query, second == kSecondArray ? 4 * kMaxInput : kMaxInput);
  const int rc0 = bce_hip_create(&in.ctx, 0);
  reader.join();
  if (second != kNoSecond) query_reader.join();
  if (in_archive && file.status == -1) { printf("Archive not found.\n"); return -1; }
  if (in_archive && (file.status != 0 || file.size() == 0)) { printf("Could not read Archive.\n"); return -2; }
  if (!in_archive && (file.status != 0 || file.size() == 0 || file.size() >= kMaxInput)) { printf("Error loading file\n"); return -1; }
  if (in_archive && in.one_text && is_container(file)) { printf("A container holds separate texts, each with a suffix array of its own: decode it and sort its blocks one by one\n"); return -2; }
  if (second == kSecondDelta && query.status == -1) { printf("Archive not found.\n"); return -1; }
  if (second == kSecondDelta && (query.status != 0 || !read_delta_header(query.data(), query.size(), in.dh))) { printf("Could not read Archive.\n"); return -2; }
  if (second == kSecondQuery && (query.status != 0 || query.size() == 0 || query.size() >= kMaxInput)) { printf("Error loading file\n"); return -1; }
  if (second == kSecondArray && (query.status == -1 || query.status == -2)) { printf("Error loading file\n"); return -1; }
  if (second == kSecondArray && query.size() != 4 * file.size()) {
    printf("%s holds %zu bytes: the suffix array of the %zu bytes of %s has %zu\n", second_path, query.size(), file.size(), path, 4 * file.size());
    return -2;
  }
  if (rc0 != 0 || !bce_hip_count || !have_api) { printf("No usable HIP device: %s\n", bce_hip_strerror(rc0 ? rc0 : BCE_HIP_E_DEVICE)); return -3; }
  in.text = file.data();
  in.n = file.size();
  if (!in_archive) return 0;
  std::vector<std::pair<size_t, size_t>> blocks;
  if (!archive_blocks(file, blocks)) { printf("Could not read Archive.\n"); return -2; }
  const bool checked = container_version(file) == 2;
  std::vector<size_t> at(blocks.size() + 1, 0);
  for (size_t b = 0; b < blocks.size(); ++b) {                      // sizes from the blocks' own headers, which a container's table must name (as -d)
    size_t hn = 0;
    const int hr = bce_hip_decompress(file.data() + blocks[b].first, blocks[b].second, nullptr, 0, &hn);
    if (hr != 0 && blocks.size() == 1 && !is_container(file)) { printf("Decompression failed: %s\n", bce_hip_strerror(hr)); return -4; }
    if (hr != 0 || hn < 1 || hn >= kMaxInput || (is_container(file) && (uint64_t)hn != table_raw(file, b))) { printf("Could not read Archive.\n"); return -2; }
    at[b + 1] = at[b] + hn;
    if (at[b + 1] >= kMaxInput) { printf("The archive holds 2^31 bytes or more: one index covers one text below that\n"); return -2; }
  }
  if (checked && !bce_hip_decompress_device_crc32) { printf("No usable HIP device: %s\n", bce_hip_strerror(BCE_HIP_E_DEVICE)); return -3; }
  in.decoded.resize(at.back());
  for (size_t b = 0; b < blocks.size(); ++b) {
    const uint8_t *ap = file.data() + blocks[b].first;
    const size_t want = at[b + 1] - at[b];
    size_t got = 0;
    uint32_t crc = 0;
    int rc = checked ? bce_hip_decompress_device_crc32(in.ctx, ap, blocks[b].second, in.decoded.data() + at[b], want, &got, &crc)
                     : bce_hip_decompress_device(in.ctx, ap, blocks[b].second, in.decoded.data() + at[b], want, &got);
    if (rc == 0 && got != want) rc = BCE_HIP_E_INTERNAL;
    if (rc != 0) {
      if (bce_hip_last_error(in.ctx)[0]) printf("%s\n", bce_hip_last_error(in.ctx));
      printf("Decompression failed: %s\n", bce_hip_strerror(rc));
      return -4;
    }
    if (checked && crc != table_crc(file, b)) { print_mismatch(b, table_crc(file, b), crc); return -4; }
  }
  in.text = in.decoded.data();
  in.n = in.decoded.size();
  return 0;
}
// the text into the context and indexed: K1, K2
static int index_text(const IndexInput &in) {
  int rc = bce_hip_load_host(in.ctx, in.text, (uint32_t)in.n);
  if (rc == 0) rc = bce_hip_bwt(in.ctx, nullptr);
  if (rc == 0) rc = bce_hip_build_planes(in.ctx, nullptr);
  return rc;
}
static int index_failed(const IndexInput &in, const char *what, int rc) {
  printf("%s failed: %s (%s)\n", what, bce_hip_strerror(rc), bce_hip_last_error(in.ctx));
  return -4;
}
static int index_done(IndexInput &in) {
  in.ctx = nullptr;                                                   // (left to fast_exit, like -d)
  fast_exit(0);
  return 0;
}

// -g / -gd
static int count_command(const char *pattern, const char *path, bool in_archive) {
  IndexInput in;
  if (const int ec = index_open(in, path, in_archive, nullptr, kNoSecond, true)) return ec;
  const size_t m = strlen(pattern);
  const uint8_t *pat = reinterpret_cast<const uint8_t *>(pattern);
  uint64_t count = 0;
  if (m <= in.n) {                                                  // (a longer pattern occurs nowhere in the text, only around it)
    const uint64_t offsets[2] = {0, m};
    int rc = index_text(in);
    if (rc == 0) rc = bce_hip_count(in.ctx, pat, offsets, 1, &count);
    if (rc != 0) return index_failed(in, "Count", rc);
    count -= seam_matches(in.text, in.n, pat, m);
  }
  printf("%llu occurrences\n", (unsigned long long)count);
  return index_done(in);
}

// -gl / -gld
static int locate_command(const char *pattern, const char *path, bool in_archive) {
  IndexInput in;
  if (const int ec = index_open(in, path, in_archive, nullptr, kNoSecond, bce_hip_locate != nullptr)) return ec;
  const size_t m = strlen(pattern);
  const uint8_t *pat = reinterpret_cast<const uint8_t *>(pattern);
  uint64_t count = 0;
  std::vector<uint32_t> where;
  if (m <= in.n) {                                                  // (as -g)
    const uint64_t offsets[2] = {0, m};
    uint64_t hits[2] = {0, 0};
    int rc = index_text(in);
    if (rc == 0) rc = bce_hip_locate(in.ctx, pat, offsets, 1, BCE_HIP_LOCATE_LINEAR, hits, nullptr, 0, &count);   // how many
    if (rc == 0 && count) {
      where.resize(count);
      rc = bce_hip_locate(in.ctx, pat, offsets, 1, BCE_HIP_LOCATE_LINEAR, hits, where.data(), count, &count);
    }
    if (rc != 0) return index_failed(in, "Locate", rc);
  }
  for (uint32_t at : where) printf("%u\n", at);
  printf("%llu occurrences\n", (unsigned long long)count);
  return index_done(in);
}

// -gn / -gnd: the hits of -g with up to K bytes different, per distance.  bce_hip_count_near counts them in the circular text; the
// windows that start in the text's last m - 1 bytes and run into its first come off here, each at its own distance.
static int count_near_command(uint32_t K, const char *pattern, const char *path, bool in_archive) {
  IndexInput in;
  if (const int ec = index_open(in, path, in_archive, nullptr, kNoSecond, bce_hip_count_near != nullptr)) return ec;
  const size_t m = strlen(pattern);
  const uint8_t *pat = reinterpret_cast<const uint8_t *>(pattern);
  uint64_t per[BCE_HIP_NEAR_MAX_K + 1] = {0, 0, 0}, count = 0;
  if (m <= in.n) {                                                  // (as -g)
    const uint64_t offsets[2] = {0, m};
    int rc = index_text(in);
    if (rc == 0) rc = bce_hip_count_near(in.ctx, pat, offsets, 1, K, per);
    if (rc != 0) return index_failed(in, "Count", rc);
    for (size_t at = in.n - m + 1; at < in.n; ++at) {
      uint32_t d = 0;
      for (size_t j = 0; j < m && d <= K; ++j) d += pat[j] != in.text[at + j < in.n ? at + j : at + j - in.n];
      if (d <= K) per[d] -= 1;
    }
  }
  for (uint32_t d = 0; d <= K; ++d) {
    printf("distance %u: %llu\n", d, (unsigned long long)per[d]);
    count += per[d];
  }
  printf("%llu occurrences\n", (unsigned long long)count);
  return index_done(in);
}

// -gnl / -gnld: the linear hits of bce_hip_locate_near, "POS d" per line in ascending position, before the count line
static int locate_near_command(uint32_t K, const char *pattern, const char *path, bool in_archive) {
  IndexInput in;
  if (const int ec = index_open(in, path, in_archive, nullptr, kNoSecond, bce_hip_locate_near != nullptr)) return ec;
  const size_t m = strlen(pattern);
  const uint8_t *pat = reinterpret_cast<const uint8_t *>(pattern);
  uint64_t count = 0;
  std::vector<uint32_t> where;
  std::vector<uint8_t> dist;
  if (m <= in.n) {                                                  // (as -g)
    const uint64_t offsets[2] = {0, m};
    uint64_t hits[2] = {0, 0};
    int rc = index_text(in);
    if (rc == 0) rc = bce_hip_locate_near(in.ctx, pat, offsets, 1, K, BCE_HIP_LOCATE_LINEAR, hits, nullptr, nullptr, 0, &count);   // how many
    if (rc == 0 && count) {
      where.resize(count);
      dist.resize(count);
      rc = bce_hip_locate_near(in.ctx, pat, offsets, 1, K, BCE_HIP_LOCATE_LINEAR, hits, where.data(), dist.data(), count, &count);
    }
    if (rc != 0) return index_failed(in, "Locate", rc);
  }
  for (size_t r = 0; r < where.size(); ++r) printf("%u %u\n", where[r], (unsigned)dist[r]);
  printf("%llu occurrences\n", (unsigned long long)count);
  return index_done(in);
}

// -gw / -gwd: the positions within K edits of PATTERN (the anchored edit distance of include/bce_hip.h), per distance.  Linear
// semantics, as -g: bce_hip_count_edit restricts the alignments to those that end inside the text on the GPU, nothing is corrected
// here.  The pattern's length is not judged against the text's: a shorter alignment may still fit.
static int count_edit_command(uint32_t K, const char *pattern, const char *path, bool in_archive) {
  IndexInput in;
  if (const int ec = index_open(in, path, in_archive, nullptr, kNoSecond, bce_hip_count_edit != nullptr)) return ec;
  const size_t m = strlen(pattern);
  const uint64_t offsets[2] = {0, m};
  uint64_t per[BCE_HIP_EDIT_MAX_K + 1] = {0, 0, 0}, count = 0;
  int rc = index_text(in);
  if (rc == 0) rc = bce_hip_count_edit(in.ctx, reinterpret_cast<const uint8_t *>(pattern), offsets, 1, K, BCE_HIP_LOCATE_LINEAR, per);
  if (rc != 0) return index_failed(in, "Count", rc);
  for (uint32_t d = 0; d <= K; ++d) {
    printf("distance %u: %llu\n", d, (unsigned long long)per[d]);
    count += per[d];
  }
  printf("%llu occurrences\n", (unsigned long long)count);
  return index_done(in);
}

// -gwl / -gwld: the linear hits of bce_hip_locate_edit, "POS LEN d" per line in ascending position, before the count line
static int locate_edit_command(uint32_t K, const char *pattern, const char *path, bool in_archive) {
  IndexInput in;
  if (const int ec = index_open(in, path, in_archive, nullptr, kNoSecond, bce_hip_locate_edit != nullptr)) return ec;
  const uint64_t offsets[2] = {0, strlen(pattern)};
  const uint8_t *pat = reinterpret_cast<const uint8_t *>(pattern);
  uint64_t count = 0, hits[2] = {0, 0};
  std::vector<uint32_t> where;
  std::vector<uint16_t> lens;
  std::vector<uint8_t> dist;
  int rc = index_text(in);
  if (rc == 0) rc = bce_hip_locate_edit(in.ctx, pat, offsets, 1, K, BCE_HIP_LOCATE_LINEAR, hits, nullptr, nullptr, nullptr, 0, &count);   // how many
  if (rc == 0 && count) {
    where.resize(count);
    lens.resize(count);
    dist.resize(count);
    rc = bce_hip_locate_edit(in.ctx, pat, offsets, 1, K, BCE_HIP_LOCATE_LINEAR, hits, where.data(), lens.data(), dist.data(), count, &count);
  }
  if (rc != 0) return index_failed(in, "Locate", rc);
  for (size_t r = 0; r < where.size(); ++r) printf("%u %u %u\n", where[r], (unsigned)lens[r], (unsigned)dist[r]);
  printf("%llu occurrences\n", (unsigned long long)count);
  return index_done(in);
}

// -ge[i] / -ge[i]d / -ge[i]l / -ge[i]ld: the hits of an expression of byte classes (class_expr.h), one 256-bit set per position, under
// the default budget of search nodes.  Linear semantics, as -g: bce_hip_count_classes counts in the circular text and the windows
// that start in the text's last m - 1 bytes and match come off here; bce_hip_locate_classes filters on the GPU.  A search that runs
// out of its budget says so and nothing else.
static const int kExitGaveUp = 1;
static int classes_command(const std::vector<uint32_t> &masks, bool list, const char *path, bool in_archive) {
  IndexInput in;
  if (const int ec = index_open(in, path, in_archive, nullptr, kNoSecond, list ? bce_hip_locate_classes != nullptr : bce_hip_count_classes != nullptr)) return ec;
  const size_t m = masks.size() / 8;
  uint64_t count = 0;
  std::vector<uint32_t> where;
  if (m <= in.n) {                                                  // (as -g)
    const uint64_t offsets[2] = {0, m};
    uint64_t hits[2] = {0, 0};
    uint32_t status = 0;
    int rc = index_text(in);
    if (rc == 0 && list) {
      rc = bce_hip_locate_classes(in.ctx, masks.data(), offsets, 1, 0, BCE_HIP_LOCATE_LINEAR, hits, &status, nullptr, 0, &count);   // how many
      if (rc == 0 && count) {
        where.resize(count);
        rc = bce_hip_locate_classes(in.ctx, masks.data(), offsets, 1, 0, BCE_HIP_LOCATE_LINEAR, hits, &status, where.data(), count, &count);
      }
    } else if (rc == 0) {
      rc = bce_hip_count_classes(in.ctx, masks.data(), offsets, 1, 0, &count, nullptr, &status);
    }
    if (rc != 0) return index_failed(in, list ? "Locate" : "Count", rc);
    if (status == BCE_HIP_CLASS_OVER) {
      printf("search gave up: more than %u partial matches\n", BCE_HIP_CLASS_DEFAULT_NODES);
      return kExitGaveUp;
    }
    for (size_t at = in.n - m + 1; !list && at < in.n; ++at) {
      size_t j = 0;
      while (j < m) {
        const uint8_t c = in.text[at + j < in.n ? at + j : at + j - in.n];
        if (!((masks[8 * j + (c >> 5)] >> (c & 31)) & 1u)) break;
        ++j;
      }
      count -= j == m;
    }
  }
  for (uint32_t at : where) printf("%u\n", at);
  printf("%llu occurrences\n", (unsigned long long)count);
  return index_done(in);
}

// -gm / -gmd
static int coverage_command(uint32_t min_len, const char *path, bool in_archive, const char *query_path) {
  IndexInput in;
  if (const int ec = index_open(in, path, in_archive, query_path, kSecondQuery, bce_hip_coverage != nullptr)) return ec;
  const HostFile &query = in.second;
  uint64_t covered = 0;
  int rc = index_text(in);
  if (rc == 0) rc = bce_hip_coverage(in.ctx, query.data(), query.size(), min_len, BCE_HIP_MATCH_LINEAR, &covered);
  if (rc != 0) return index_failed(in, "Match", rc);
  printf("%llu of %zu bytes (%.1f %%) of %s lie in strings of %u bytes or more that occur in %s\n", (unsigned long long)covered, query.size(),
         100.0 * (double)covered / (double)query.size(), query_path, min_len, path);
  return index_done(in);
}

// -gz / -gzd: the file or archive is read, judged, decoded and indexed as for the others; the text is parsed against itself on the GPU
// (bce_hip_self_parse at the bounds MINLEN and max(256, MINLEN), a sizing call: only the four counts come back) and one line printed.
static int self_command(uint32_t min_len, const char *path, bool in_archive) {
  IndexInput in;
  if (const int ec = index_open(in, path, in_archive, nullptr, kNoSecond, bce_hip_self_parse != nullptr)) return ec;
  const uint32_t max_len = min_len > kDeltaMaxLen ? min_len : kDeltaMaxLen;
  bce_hip_parse_info info{};
  int rc = index_text(in);
  if (rc == 0) rc = bce_hip_self_parse(in.ctx, min_len, max_len, nullptr, 0, nullptr, 0, &info);
  if (rc != 0) return index_failed(in, "Self-parse", rc);
  printf("%llu copies of %llu bytes, %llu literal bytes in %llu runs: %llu phrases at bounds %u .. %u; %llu of %zu bytes repeat earlier text\n",
         (unsigned long long)info.ncopies, (unsigned long long)info.copied, (unsigned long long)info.nlits, (unsigned long long)(info.nops - info.ncopies),
         (unsigned long long)(info.ncopies + info.nlits), min_len, max_len, (unsigned long long)info.copied, in.n);
  return index_done(in);
}

// -gs / -gsd: the file or archive is read, judged and decoded as for the others (a container is refused: its blocks are separate
// texts); the text is sorted on the GPU (bce_hip_suffix_array) and its n rows written as native 32-bit words, the layout of
// libdivsufsort's mksary.  A write that fails leaves no file.
static int sa_command(const char *path, bool in_archive, const char *out_path) {
  IndexInput in;
  in.one_text = true;
  if (const int ec = index_open(in, path, in_archive, nullptr, kNoSecond, bce_hip_suffix_array != nullptr)) return ec;
  if (in.n >= kMaxInput - 1) { printf("Error loading file\n"); return -1; }   // (the sort adds a sentinel: n < 2^31 - 1)
  std::vector<uint32_t> sa(in.n);
  const int rc = bce_hip_suffix_array(in.ctx, in.text, (uint32_t)in.n, sa.data(), nullptr);
  if (rc != 0) return index_failed(in, "Suffix sort", rc);
  if (!write_file(out_path, sa.data(), sa.size() * 4)) { remove(out_path); printf("Could not write file.\n"); return -5; }
  printf("%zu suffixes\n", in.n);
  return index_done(in);
}

// -gsc: the file, then the array (4 n bytes), then the device; checked on the GPU (bce_hip_sufcheck).  One line; exit status 0 =
// sorted, kExitDiffers = not.
static int sa_check_command(const char *path, const char *sa_path) {
  IndexInput in;
  if (const int ec = index_open(in, path, false, sa_path, kSecondArray, bce_hip_sufcheck != nullptr)) return ec;
  uint64_t bad = 0;
  uint32_t reason = 0;
  const int rc = bce_hip_sufcheck(in.ctx, in.text, reinterpret_cast<const uint32_t *>(in.second.data()), (uint32_t)in.n, &bad, &reason);
  if (rc != 0) return index_failed(in, "Suffix check", rc);
  const uint32_t *sa = reinterpret_cast<const uint32_t *>(in.second.data());
  switch (reason) {
    case BCE_HIP_SUFCHECK_OK: printf("%zu suffixes in order\n", in.n); return index_done(in);
    case BCE_HIP_SUFCHECK_RANGE: printf("Out of range: row %llu holds %u, the text has %zu bytes\n", (unsigned long long)bad, sa[bad], in.n); break;
    case BCE_HIP_SUFCHECK_MISSING: printf("Not a permutation: no row holds position %llu\n", (unsigned long long)bad); break;
    default: printf("Out of order: row %llu (suffix %u) sorts before row %llu (suffix %u)\n", (unsigned long long)bad, sa[bad], (unsigned long long)bad - 1, sa[bad - 1]); break;
  }
  return kExitDiffers;
}

// -gk / -gkd: k = 0 .. K, and K + 1 for H_K
static int kgrams_command(uint32_t K, const char *path, bool in_archive) {
  IndexInput in;
  if (const int ec = index_open(in, path, in_archive, nullptr, kNoSecond, bce_hip_kgrams && bce_hip_longest_repeat)) return ec;
  uint32_t ks[kMaxKgramOrder + 2];
  bce_hip_kgram rec[kMaxKgramOrder + 2];
  for (uint32_t k = 0; k < K + 2; ++k) ks[k] = k;
  uint32_t len = 0, pos_a = 0, pos_b = 0;
  int rc = index_text(in);
  if (rc == 0) rc = bce_hip_kgrams(in.ctx, ks, K + 2, rec);
  if (rc == 0) rc = bce_hip_longest_repeat(in.ctx, BCE_HIP_MATCH_MAX_LEN, &len, &pos_a, &pos_b);
  if (rc != 0) return index_failed(in, "K-grams", rc);
  printf("k-grams of the circular text: k distinct once most H_k\n");
  for (uint32_t k = 0; k <= K; ++k) {
    const uint64_t a = rec[k].nlogn_q24, b = rec[k + 1].nlogn_q24;
    const double h = (double)(a > b ? a - b : 0) / ((double)in.n * 16777216.0);
    printf("%u %llu %llu %u %.6f\n", k, (unsigned long long)rec[k].distinct, (unsigned long long)rec[k].once, rec[k].max_count, h);
  }
  if (len == 0) printf("longest repeat: none\n");
  else if (len >= BCE_HIP_MATCH_MAX_LEN) printf("longest repeat: %u or more bytes at %u and %u\n", len, pos_a, pos_b);
  else printf("longest repeat: %u bytes at %u and %u\n", len, pos_a, pos_b);
  printf("%zu bytes\n", in.n);
  return index_done(in);
}

// -gf / -gfd
static int top_command(uint32_t K, uint32_t N, const char *path, bool in_archive) {
  IndexInput in;
  if (const int ec = index_open(in, path, in_archive, nullptr, kNoSecond, bce_hip_top_kgrams != nullptr)) return ec;
  std::vector<bce_hip_top_kgram> ent(N);                              // (at most 65536 entries of 256 bytes: 16 MB)
  std::vector<uint8_t> gram((size_t)N * K);
  uint32_t found = 0;
  uint64_t distinct = 0;
  int rc = index_text(in);
  if (rc == 0) rc = bce_hip_top_kgrams(in.ctx, K, N, ent.data(), gram.data(), gram.size(), &found, &distinct, nullptr);
  if (rc != 0) return index_failed(in, "Top k-grams", rc);
  printf("most frequent %u-grams of the circular text: count position bytes\n", K);
  std::string line;
  for (uint32_t e = 0; e < found; ++e) {
    line.clear();
    char esc[5];
    for (uint32_t j = 0; j < K; ++j) { bce::top_escape(gram[(size_t)e * K + j], esc); line += esc; }
    printf("%u %u %s\n", ent[e].count, ent[e].pos, line.c_str());
  }
  printf("%llu distinct, %zu bytes\n", (unsigned long long)distinct, in.n);
  return index_done(in);
}

// -gp / -gpd: the maximal repeats of MINLEN bytes or more at the search bound 4096, the N heaviest in ORDER.  A head line, one line
// per repeat -- its length ("4096+": that many or more), its occurrences, the position of one, its first 64 bytes in top_escape's
// escaping ("..." behind a longer one) -- then the counts, the runs of the BWT and the text's size.
constexpr uint32_t kMaxRepShown = 64;
static const char *const kMaxRepOrders[3] = {"len", "count", "gain"};
static int parse_maxrep_order(const char *s) {
  for (int o = 0; o < 3; ++o) if (strcmp(s, kMaxRepOrders[o]) == 0) return o;
  return -1;
}
static int maxrep_command(uint32_t order, uint32_t min_len, uint32_t N, const char *path, bool in_archive) {
  IndexInput in;
  if (const int ec = index_open(in, path, in_archive, nullptr, kNoSecond, bce_hip_maximal_repeats != nullptr)) return ec;
  std::vector<bce_hip_maxrep> ent(N);
  std::vector<uint8_t> str((size_t)N * kMaxRepShown);
  bce_hip_maxrep_info info{};
  int rc = index_text(in);
  if (rc == 0) rc = bce_hip_maximal_repeats(in.ctx, min_len, BCE_HIP_MATCH_MAX_LEN, order, N, ent.data(), str.data(), kMaxRepShown, str.size(), &info);
  if (rc != 0) return index_failed(in, "Maximal repeats", rc);
  printf("maximal repeats of the circular text by %s: length count position bytes\n", kMaxRepOrders[order]);
  std::string line;
  for (uint32_t e = 0; e < info.found; ++e) {
    line.clear();
    char esc[5];
    const uint32_t shown = ent[e].len < kMaxRepShown ? ent[e].len : kMaxRepShown;
    for (uint32_t j = 0; j < shown; ++j) { bce::top_escape(str[(size_t)e * kMaxRepShown + j], esc); line += esc; }
    if (ent[e].len > kMaxRepShown) line += "...";
    printf("%u%s %u %u %s\n", ent[e].len, ent[e].len >= BCE_HIP_MATCH_MAX_LEN ? "+" : "", ent[e].count, ent[e].pos, line.c_str());
  }
  printf("%llu maximal repeats of %u bytes or more (%llu of %u or more), %llu BWT runs, %zu bytes\n", (unsigned long long)info.total, min_len,
         (unsigned long long)info.capped, BCE_HIP_MATCH_MAX_LEN, (unsigned long long)info.bwt_runs, in.n);
  return index_done(in);
}

// -gr / -grd
static int delta_command(uint32_t min_len, const char *path, bool in_archive, const char *query_path, const char *out_path) {
  IndexInput in;
  if (const int ec = index_open(in, path, in_archive, query_path, kSecondQuery, bce_hip_parse && bce_hip_input_crc32 && bce_hip_coverage)) return ec;
  const HostFile &query = in.second;
  const uint32_t max_len = min_len > kDeltaMaxLen ? min_len : kDeltaMaxLen;
  bce_hip_parse_info info{};
  DeltaHeader h{};
  int rc = index_text(in);
  if (rc == 0) rc = bce_hip_input_crc32(in.ctx, &h.base_crc);
  if (rc == 0) rc = bce_hip_parse(in.ctx, query.data(), query.size(), min_len, max_len, nullptr, 0, nullptr, 0, &info);   // how much
  std::vector<uint8_t> blob;
  if (rc == 0) {
    blob.resize(kDeltaHeader + info.nops * 8 + info.nlits);
    rc = bce_hip_parse(in.ctx, query.data(), query.size(), min_len, max_len, reinterpret_cast<bce_hip_op *>(blob.data() + kDeltaHeader), info.nops,
                       blob.data() + kDeltaHeader + info.nops * 8, info.nlits, &info);
  }
  if (rc != 0) return index_failed(in, "Parse", rc);
  h.n = in.n; h.q = query.size(); h.crc = bce_hip_crc32(0, query.data(), query.size()); h.min_len = min_len; h.max_len = max_len;
  h.nops = info.nops; h.nlits = info.nlits;
  write_delta_header(blob.data(), h);
  if (!write_file(out_path, blob.data(), blob.size())) { printf("Could not write Archive.\n"); return -5; }
  printf("%llu copies of %llu bytes, %llu literal bytes in %llu runs: %zu bytes of delta\n", (unsigned long long)info.ncopies,
         (unsigned long long)info.copied, (unsigned long long)info.nlits, (unsigned long long)(info.nops - info.ncopies), blob.size());
  return index_done(in);
}

// -ga / -gad: the base is loaded, not indexed
static int apply_command(const char *path, bool in_archive, const char *delta_path, const char *out_path) {
  IndexInput in;
  if (const int ec = index_open(in, path, in_archive, delta_path, kSecondDelta, bce_hip_patch && bce_hip_input_crc32 && bce_hip_coverage)) return ec;
  const HostFile &delta = in.second;
  const DeltaHeader &dh = in.dh;
  const bce_hip_op *ops = reinterpret_cast<const bce_hip_op *>(delta.data() + kDeltaHeader);   // (56 bytes behind an allocation's start: aligned)
  const uint8_t *lits = delta.data() + kDeltaHeader + dh.nops * 8;
  if (in.n != dh.n) { printf("The delta was made against %llu bytes, not %zu\n", (unsigned long long)dh.n, in.n); return kExitDiffers; }
  uint32_t crc = 0;
  int rc = bce_hip_load_host(in.ctx, in.text, (uint32_t)in.n);
  if (rc == 0) rc = bce_hip_input_crc32(in.ctx, &crc);
  if (rc != 0) return index_failed(in, "Patch", rc);
  if (crc != dh.base_crc) { printf("Checksum mismatch in the base: delta %08X, file %08X\n", dh.base_crc, crc); return kExitDiffers; }
  uint64_t total = 0;
  rc = bce_hip_patch(in.ctx, ops, dh.nops, lits, dh.nlits, nullptr, 0, &total);          // judged on the GPU, and how much
  if (rc == BCE_HIP_E_ARG || (rc == 0 && total != dh.q)) { printf("Could not read Archive.\n"); return -2; }
  std::vector<uint8_t> out((size_t)total);
  if (rc == 0 && total) rc = bce_hip_patch(in.ctx, ops, dh.nops, lits, dh.nlits, out.data(), total, &total);
  if (rc != 0) return index_failed(in, "Patch", rc);
  crc = bce_hip_crc32(0, out.data(), out.size());
  if (crc != dh.crc) { printf("Checksum mismatch in the result: delta %08X, rebuilt %08X\n", dh.crc, crc); return kExitDiffers; }
  if (!write_file(out_path, out.data(), out.size())) { printf("Could not write file.\n"); return -5; }
  printf("Rebuilt %zu B from %zu B and a delta of %zu B\n", out.size(), in.n, delta.size());
  return index_done(in);
}

// MINLEN of -gm / -gmd: decimal digits only, 1 .. 4096 (BCE_HIP_MATCH_MAX_LEN); anything else: 0
static uint32_t parse_min_len(const char *s) {
  uint32_t v = 0;
  if (!*s) return 0;
  for (; *s; ++s) {
    if (*s < '0' || *s > '9') return 0;
    v = v * 10 + (uint32_t)(*s - '0');
    if (v > BCE_HIP_MATCH_MAX_LEN) return 0;
  }
  return v;
}

// K of -gn / -gnl: one decimal digit, 0 .. 2 (BCE_HIP_NEAR_MAX_K); anything else: -1
static int parse_near_k(const char *s) {
  return s[0] >= '0' && s[0] <= (char)('0' + BCE_HIP_NEAR_MAX_K) && s[1] == 0 ? s[0] - '0' : -1;
}

// the letters behind -ge: i, l, d, each at most once and in that order; anything else: false
static bool parse_class_option(const char *s, bool &ignore_case, bool &list, bool &in_archive) {
  if (strncmp(s, "-ge", 3) != 0) return false;
  s += 3;
  ignore_case = *s == 'i'; s += ignore_case;
  list = *s == 'l'; s += list;
  in_archive = *s == 'd'; s += in_archive;
  return *s == 0;
}

// K of -gk / -gkd: decimal digits only, 0 .. 32; anything else: -1
static int parse_order(const char *s) {
  uint32_t v = 0;
  if (!*s) return -1;
  for (; *s; ++s) {
    if (*s < '0' || *s > '9') return -1;
    v = v * 10 + (uint32_t)(*s - '0');
    if (v > kMaxKgramOrder) return -1;
  }
  return (int)v;
}

// K of -gf / -gfd (1 .. 256) and its N (1 .. 65536): decimal digits only; anything else: 0
static uint32_t parse_count(const char *s, uint32_t most) {
  uint32_t v = 0;
  if (!*s) return 0;
  for (; *s; ++s) {
    if (*s < '0' || *s > '9') return 0;
    v = v * 10 + (uint32_t)(*s - '0');
    if (v > most) return 0;
  }
  return v;
}

static int usage() {
  printf("Usage:\n");
  printf("  bce -c archive.bce file [config.bcc]\n");
  printf("   Compresses \"file\" to archive \"archive.bce\" [using config \"config.bcc\"]\n");
  printf("\n");
  printf("  bce -d file archive.bce\n");
  printf("   Decompresses archive \"archive.bce\" to \"file\"\n");
  printf("\n");
  printf("  bce -s config.bcc file\n");
  printf("   Scan \"file\" and generate a config file \"config.bcc\" to improve the AdaptiveCoder (uses a lot of memory)\n");
  printf("\n");
  printf("  bce -t file archive.bce\n");
  printf("   Tests archive \"archive.bce\" against \"file\": decodes it on the GPU and compares there, writes nothing (extension; exit status 0 = equal, %d = differs)\n", kExitDiffers);
  printf("\n");
  printf("  bce -cN archive.bcem file [config.bcc]      (extension: N = 2..64 blocks, one container, all GPUs of the node; every block < 2^31 bytes)\n");
  printf("\n");
  printf("  bce -CN archive.bcem file [config.bcc]\n");
  printf("   As -cN with N = 1..64, and the container holds the CRC-32 of every block: -d and -ds check what they decode (extension)\n");
  printf("\n");
  printf("  bce -t archive.bcem\n");
  printf("   Tests a -CN archive against its own checksums: decodes it on the GPU, writes nothing (extension; exit status 0 = sound, %d = a block differs, %d = the archive carries no checksum)\n", kExitDiffers, kExitNoChecksum);
  printf("\n");
  printf("  bce -e file [config.bcc]\n");
  printf("   Estimates the size -c would give for \"file\" [using config \"config.bcc\"]: the model's code lengths are summed on the GPU, nothing is coded or written (extension)\n");
  printf("\n");
  printf("  bce -gw K PATTERN file\n");
  printf("   Counts the positions of \"file\" where something starts that is within K (0..2) edits of PATTERN -- bytes substituted, inserted or deleted between PATTERN's first and last byte, which stay aligned: one line \"distance d: N\" for d = 0..K, each position under its least distance, then the sum; backward search that branches three ways, reduced per position through the suffix array, on the GPU (extension)\n");
  printf("\n");
  printf("  bce -gwd K PATTERN archive.bce\n");
  printf("   The same counts in what \"archive.bce\" (or a -cN / -CN container) holds, decoded on the GPU; writes nothing (extension)\n");
  printf("\n");
  printf("  bce -gwl K PATTERN file\n");
  printf("   Prints where they start: \"POS LEN d\" per hit, the byte offset, the length of the best alignment there and its number of edits, ascending by offset, then the count (extension)\n");
  printf("\n");
  printf("  bce -gwld K PATTERN archive.bce\n");
  printf("   The same lines for what \"archive.bce\" (or a -cN / -CN container) holds, decoded on the GPU; writes nothing (extension)\n");
  printf("\n");
  printf("  bce -gp ORDER MINLEN N file\n");
  printf("   Prints the N (1..65536) heaviest maximal repeats of MINLEN (1..4096) bytes or more of the circular text of \"file\": strings that occur twice or more and lose an occurrence when extended by a byte on either side.  ORDER is len (longest first), count (most frequent first) or gain (length times the occurrences after the first).  Per repeat: length (4096+: that or more), occurrences, the position of one and the first 64 bytes (\\xHH for all but printable ASCII); then their number, the runs of the BWT and the size; found, selected and sorted on the GPU (extension)\n");
  printf("\n");
  printf("  bce -gpd ORDER MINLEN N archive.bce\n");
  printf("   The same list for what \"archive.bce\" (or a -cN / -CN container) holds, decoded on the GPU; writes nothing (extension)\n");
  printf("\n");
  printf("  bce -gs file out.sa\n");
  printf("   Writes the suffix array of \"file\" to \"out.sa\": one native 32-bit word per suffix in sorted order (the layout of libdivsufsort's mksary), sorted on the GPU (extension)\n");
  printf("\n");
  printf("  bce -gsd archive.bce out.sa\n");
  printf("   The same array for what \"archive.bce\" holds, decoded on the GPU; a -cN / -CN container is refused, its blocks are separate texts (extension)\n");
  printf("\n");
  printf("  bce -gsc file in.sa\n");
  printf("   Checks on the GPU, in linear time, that \"in.sa\" is the suffix array of \"file\" (extension; exit status 0 = in order, %d = not: the line names the row or the position)\n", kExitDiffers);
  printf("\n");
  printf("  bce -ge[i] EXPR file\n");
  printf("   Counts how often something occurs in \"file\" that EXPR describes byte by byte: . is any byte, [a-f0-9] a set with ranges, [^...] its complement, \\xHH a byte in hex, \\ before one of \\ . [ ] ^ - { } that byte, {N} after any of these the same N (1..4096) times, every other byte itself; with i letters match both cases. Backward search that branches at every set, on the GPU; a search of more than %u partial matches gives up: \"search gave up\", exit status %d (extension)\n", BCE_HIP_CLASS_DEFAULT_NODES, kExitGaveUp);
  printf("\n");
  printf("  bce -ge[i]d EXPR archive.bce\n");
  printf("   The same count in what \"archive.bce\" (or a -cN / -CN container) holds, decoded on the GPU; writes nothing (extension)\n");
  printf("\n");
  printf("  bce -ge[i]l EXPR file\n");
  printf("   Prints where they occur: the byte offsets, one per line, ascending, then the count (extension)\n");
  printf("\n");
  printf("  bce -ge[i]ld EXPR archive.bce\n");
  printf("   The same offsets in what \"archive.bce\" (or a -cN / -CN container) holds, decoded on the GPU; writes nothing (extension)\n");
  printf("\n");
  printf("  bce -g PATTERN file\n");
  printf("   Counts how often the bytes of PATTERN occur in \"file\", overlapping matches included: the file is indexed on the GPU and the count comes from the index (extension)\n");
  printf("\n");
  printf("  bce -gd PATTERN archive.bce\n");
  printf("   The same count in what \"archive.bce\" (or a -cN / -CN container) holds, decoded on the GPU; writes nothing (extension)\n");
  printf("\n");
  printf("  bce -gz MINLEN file\n");
  printf("   Prints how \"file\" parses into copies of MINLEN (1..4096) bytes or more of its OWN earlier bytes plus the bytes that are new: copies, literal bytes and runs, the phrase count (with MINLEN 1 the LZ77 measure z) and how many bytes repeat earlier text; longest previous factors and the chain are computed on the GPU (extension)\n");
  printf("\n");
  printf("  bce -gzd MINLEN archive.bce\n");
  printf("   The same line for what \"archive.bce\" (or a -cN / -CN container) holds, decoded on the GPU; writes nothing (extension)\n");
  printf("\n");
  printf("  bce -gl PATTERN file\n");
  printf("   Prints where the bytes of PATTERN occur in \"file\": the byte offsets, one per line, ascending, then the count; they come from the index and the suffix array on the GPU (extension)\n");
  printf("\n");
  printf("  bce -gn K PATTERN file\n");
  printf("   Counts how often something occurs in \"file\" that differs from PATTERN in at most K (0..2) bytes: one line \"distance d: N\" for d = 0..K, then the sum; backward search that branches at every allowed mismatch, on the GPU (extension)\n");
  printf("\n");
  printf("  bce -gnd K PATTERN archive.bce\n");
  printf("   The same counts in what \"archive.bce\" (or a -cN / -CN container) holds, decoded on the GPU; writes nothing (extension)\n");
  printf("\n");
  printf("  bce -gnl K PATTERN file\n");
  printf("   Prints where they occur: \"POS d\" per hit, the byte offset and its number of different bytes, ascending by offset, then the count (extension)\n");
  printf("\n");
  printf("  bce -gnld K PATTERN archive.bce\n");
  printf("   The same lines for what \"archive.bce\" (or a -cN / -CN container) holds, decoded on the GPU; writes nothing (extension)\n");
  printf("\n");
  printf("  bce -gld PATTERN archive.bce\n");
  printf("   The same offsets in what \"archive.bce\" (or a -cN / -CN container) holds, decoded on the GPU; writes nothing (extension)\n");
  printf("\n");
  printf("  bce -gm MINLEN file query_file\n");
  printf("   Prints how many bytes of \"query_file\" lie in strings of MINLEN (1..4096) bytes or more that occur in \"file\": the file is indexed on the GPU and every position of the query is searched in the index there (extension)\n");
  printf("\n");
  printf("  bce -gmd MINLEN archive.bce query_file\n");
  printf("   The same figure against what \"archive.bce\" (or a -cN / -CN container) holds, decoded on the GPU; writes nothing (extension)\n");
  printf("\n");
  printf("  bce -gk K file\n");
  printf("   Prints for k = 0..K (K = 0..32) how many distinct k-grams the circular text of \"file\" has, how many occur once, how often the most frequent one occurs and the order-k entropy H_k in bits per byte, then its longest repeat: all reduced on the GPU from the LCP array of the sorted rotations (extension)\n");
  printf("\n");
  printf("  bce -gkd K archive.bce\n");
  printf("   The same figures for what \"archive.bce\" (or a -cN / -CN container) holds, decoded on the GPU; writes nothing (extension)\n");
  printf("\n");
  printf("  bce -gr MINLEN file query_file out.bcd\n");
  printf("   Writes \"query_file\" as a delta against \"file\" to \"out.bcd\": copies of MINLEN (1..4096) bytes or more out of \"file\", found in its index on the GPU and chosen there, plus the bytes that are new (extension)\n");
  printf("\n");
  printf("  bce -grd MINLEN archive.bce query_file out.bcd\n");
  printf("   The same delta against what \"archive.bce\" (or a -cN / -CN container) holds, decoded on the GPU (extension)\n");
  printf("\n");
  printf("  bce -ga file in.bcd out_file\n");
  printf("   Rebuilds \"out_file\" on the GPU from \"file\" and the delta \"in.bcd\"; the CRC-32 of \"file\" is checked before and that of the result after (extension; exit status %d = one of them differs, nothing written)\n", kExitDiffers);
  printf("\n");
  printf("  bce -gad archive.bce in.bcd out_file\n");
  printf("   The same from what \"archive.bce\" (or a -cN / -CN container) holds, decoded on the GPU (extension)\n");
  printf("\n");
  printf("  bce -gf K N file\n");
  printf("   Prints the N (1..65536) most frequent K-grams (K = 1..256) of the circular text of \"file\", most frequent first and equal counts in the order of their bytes: count, the position of one occurrence and the bytes (\\xHH for all but printable ASCII), then the number of distinct K-grams; selected and sorted on the GPU from the LCP array of the sorted rotations (extension)\n");
  printf("\n");
  printf("  bce -gfd K N archive.bce\n");
  printf("   The same list for what \"archive.bce\" (or a -cN / -CN container) holds, decoded on the GPU; writes nothing (extension)\n");
  return 0;
}

int main(int argc, char **argv) {
  printf("BCE v0.4 Release\n");
  printf("Copyright (C) 2016  Christoph Diegelmann\n");
  printf("This is free software under GNU Lesser General Public License. See <http://www.gnu.org/licenses/lgpl>\n\n");

  if ((argc == 4 || argc == 5) && argv[1][0] == '-' && (argv[1][1] == 'c' || argv[1][1] == 'C')) {
    auto start = std::chrono::high_resolution_clock::now();
    HostFile data;
    // (-cN, the extension: every BLOCK obeys the reference's n < 2^31, the file may be N times that)
    // (-CN: the same with checksums, from one block on -- `-C1` is the self-checking archive of an ordinary file)
    const bool with_crc = argv[1][1] == 'C';
    const uint32_t nb_arg = (uint32_t)atoi(argv[1] + 2), nb_min = with_crc ? 1u : 2u;
    if (with_crc && (nb_arg < 1 || nb_arg > 64)) return usage();
    const size_t file_limit = nb_arg >= nb_min && nb_arg <= 64 ? (size_t)nb_arg * (kMaxInput - 1) + 1 : kMaxInput;
    std::thread reader(read_whole_file, argv[3], &data, file_limit);  // File::File, bce.cpp:842-856 -- beside the runtime's start-up
    bce_hip_ctx *ctx = nullptr;
    uint64_t expect = 0;                                          // the file's size, if it says: what the context prepares for
    { struct stat st; if (stat(argv[3], &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0) expect = (uint64_t)st.st_size; }
    if (nb_arg >= nb_min) expect = 0;                             // (-cN, -CN: the blocks get contexts of their own)
    int rc = bce_hip_create_sized(&ctx, 0, expect);
    if (rc != 0) {
      reader.join();
      printf("No usable HIP device: %s\n", bce_hip_strerror(rc));
      return -3;
    }
    const bool cli_timing = getenv("BCE_CLI_TIMING") != nullptr;
    auto lap = [&](const char *what) {
      if (cli_timing) fprintf(stderr, "cli: %-10s %.3f s\n", what, std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - start).count());
    };
    lap("create");
    // load_config, bce.cpp:626-641.  Read and validated ONCE (on the first context): `-c` and `-cN` apply the same 288
    // bytes or, with the same message, the defaults.
    std::vector<uint8_t> cfgbuf;
    if (argc == 5) read_config(argv[4], ctx, cfgbuf);
    reader.join();
    if (data.status != 0 || data.size() == 0 || data.size() >= file_limit) {   // also covers the empty file, on which the reference crashes
      printf("Error loading file\n");
      bce_hip_destroy(ctx);
      return -1;
    }
    lap("file read");
    // `-cN` (N = 2..64, an extension): N blocks in a BCEM container, spread over the GPUs of the node
    const uint32_t nblocks = nb_arg;
    if (with_crc && data.size() < nblocks) {                        // (never a plain archive in a checked one's place)
      printf("Error loading file\n");
      bce_hip_destroy(ctx);
      return -1;
    }
    if (nblocks >= nb_min && nblocks <= 64 && data.size() >= nblocks) {
      bce_hip_destroy(ctx);
      std::vector<uint8_t> blob;
      rc = compress_blocks(data, nblocks, cfgbuf.empty() ? nullptr : cfgbuf.data(), with_crc, blob);
      if (rc != 0) { printf("Compression failed: %s\n", bce_hip_strerror(rc)); return -4; }
      std::chrono::duration<double> duration = std::chrono::high_resolution_clock::now() - start;
      if (!write_file(argv[2], blob.data(), blob.size())) { printf("Could not write Archive.\n"); return -5; }
      printf("Compressed from %zu B -> %zu B in %.1f s\n", data.size(), blob.size(), duration.count());
      fast_exit(0);
      return 0;
    }
    size_t alen = 0;
    uint64_t prog = 0;
    bce_hip_set_progress(ctx, progress, &prog);
    rc = bce_hip_compress(ctx, data.data(), (uint32_t)data.size(), nullptr, 0, &alen);
    progress_end();
    lap("compress");
    if (rc != 0) {
      printf("Compression failed: %s (%s)\n", bce_hip_strerror(rc), bce_hip_last_error(ctx));
      bce_hip_destroy(ctx);
      return -4;
    }
    std::vector<uint8_t> arch(alen);
    bce_hip_archive_copy(ctx, arch.data(), arch.size());
    auto end = std::chrono::high_resolution_clock::now();
    std::chrono::duration<double> duration = end - start;
    if (!write_file(argv[2], arch.data(), arch.size())) { printf("Could not write Archive.\n"); bce_hip_destroy(ctx); return -5; }
    printf("Compressed from %zu B -> %zu B in %.1f s\n", data.size(), arch.size(), duration.count());
    lap("written");
    fast_exit(0);
    bce_hip_destroy(ctx);
    lap("destroyed");
    return 0;
  } else if (argc == 4 && argv[1][0] == '-' && argv[1][1] == 'd') {
    // Decompress (bce.cpp:1428-1472).
    auto start = std::chrono::high_resolution_clock::now();
    HostFile adata;
    const bool use_gpu = argv[1][2] != 's';
    std::thread reader(read_whole_file, argv[3], &adata, (size_t)0); // beside the runtime's start-up (-d)
    bce_hip_ctx *ctx0 = nullptr;
    int rc0 = use_gpu ? bce_hip_create(&ctx0, 0) : 0;
    reader.join();
    const bool cli_timing = getenv("BCE_CLI_TIMING") != nullptr;
    auto lap = [&](const char *what) {
      if (cli_timing) fprintf(stderr, "cli: %-10s %.3f s\n", what, std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - start).count());
    };
    lap("create");
    if (adata.status == -1) { printf("Archive not found.\n"); if (ctx0) bce_hip_destroy(ctx0); return -1; }
    if (adata.status != 0 || adata.size() == 0) { printf("Could not read Archive.\n"); if (ctx0) bce_hip_destroy(ctx0); return -2; }
    // -d: GPU-assisted decoder (kd_decode.hip), needs the GPU like -c.  -ds (the reference's low-memory unbwt variant,
    // :1466): the plain host decoder (decoder.cpp), on purpose and by name -- there is no silent fallback.
    // A BCEM container (bce -cN, the sharded bench) is decoded block by block.
    std::vector<std::pair<size_t, size_t>> blocks;               // (offset, length) of each archive inside adata
    if (!archive_blocks(adata, blocks)) { printf("Could not read Archive.\n"); return -2; }
    const bool checked = container_version(adata) == 2;             // every block's CRC-32 is in the table: what is decoded is tested
    int rc = 0;
    // the output: plain memory, not value-initialised (a vector would write 10^8 zeroes first that the decoder overwrites)
    // (2 MB-aligned with huge pages asked for, and its pages faulted in by the kernel -- MADV_POPULATE_WRITE leaves the
    // contents alone -- on a thread beside the decoding: the last device-to-host copy lands in mapped memory)
    struct FreeDeleter { void operator()(uint8_t *q) const { free(q); } };
    std::unique_ptr<uint8_t, FreeDeleter> out;
    std::thread prefault;
    auto alloc_out = [&](size_t bytes) {
      void *q = nullptr;
      const size_t two_mb = (size_t)2 << 20, len = ((bytes ? bytes : 1) + two_mb - 1) & ~(two_mb - 1);
      if (posix_memalign(&q, two_mb, len) != 0) q = nullptr;
      out.reset(static_cast<uint8_t *>(q));
      if (q) {
        (void)madvise(q, len, MADV_HUGEPAGE);
        try { prefault = std::thread([q, len] { (void)madvise(q, len, 23 /* MADV_POPULATE_WRITE */); }); } catch (...) {}
      }
      return q != nullptr;
    };
    struct JoinOnExit { std::thread &t; ~JoinOnExit() { if (t.joinable()) t.join(); } } join_prefault{prefault};
    size_t out_size = 0;
    bce_hip_ctx *keep = nullptr;                                   // the one-block context: given back after the file is written
    if (blocks.size() == 1 && !checked) {
      uint64_t prog = 0;
      bce_hip_ctx *ctx = ctx0;
      if (use_gpu) {
        if (rc0 != 0) {
          printf("No usable HIP device: %s (bce -ds decodes on the host)\n", bce_hip_strerror(rc0));
          return -3;
        }
        bce_hip_set_progress(ctx, progress, &prog);
      }
      const uint8_t *ap = adata.data() + blocks[0].first;
      size_t n = 0;
      rc = ctx ? bce_hip_decompress_device(ctx, ap, blocks[0].second, nullptr, 0, &n) : bce_hip_decompress(ap, blocks[0].second, nullptr, 0, &n);
      if (rc == 0) {
        if (!alloc_out(n)) { printf("Could not read Archive.\n"); if (ctx) bce_hip_destroy(ctx); return -2; }
        out_size = n;
        rc = ctx ? bce_hip_decompress_device(ctx, ap, blocks[0].second, out.get(), n, &n) : bce_hip_decompress(ap, blocks[0].second, out.get(), n, &n);
      }
      if (ctx) {
        progress_end();
        if (rc != 0) { printf("%s\n", bce_hip_last_error(ctx)); bce_hip_destroy(ctx); }
        else keep = ctx;
      }
      lap("decoded");
    } else {
      // a container: the blocks are independent, their sizes are in the table -- decoded side by side, two contexts per GPU
      // (a block's decoding is mostly its eight sequential range decoders on the host) or, for -ds, up to 8 host threads
      // The table's raw sizes are untrusted 64-bit values: each must be what the block's own header says (asked without
      // an output buffer: the header is parsed, nothing is written), at least one byte and below the encoder's 2^31 limit,
      // and the output is sized from the verified values only -- a wrapping or oversized table is "Could not read Archive".
      std::vector<size_t> at(blocks.size() + 1, 0);
      for (size_t b = 0; b < blocks.size(); ++b) {
        const uint64_t raw = table_raw(adata, b);
        size_t hn = 0;
        const int hr = bce_hip_decompress(adata.data() + blocks[b].first, blocks[b].second, nullptr, 0, &hn);
        if (hr != 0 || raw < 1 || raw >= 0x80000000ull || (uint64_t)hn != raw || raw > SIZE_MAX - at[b]) {
          printf("Could not read Archive.\n");
          return -2;
        }
        at[b + 1] = at[b] + (size_t)raw;
      }
      if (!alloc_out(at.back())) { printf("Could not read Archive.\n"); return -2; }
      out_size = at.back();
      std::vector<bce_hip_ctx *> ctxs;
      if (use_gpu) {
        int ndev = 0;
        for (int dev = 0; dev < 64 && ctxs.size() < blocks.size(); ++dev) {
          bce_hip_ctx *c = dev == 0 ? ctx0 : nullptr;
          if (!c && bce_hip_create(&c, dev) != 0) break;
          ctxs.push_back(c);
          ndev = dev + 1;
        }
        if (ctxs.empty()) { printf("No usable HIP device (bce -ds decodes on the host)\n"); return -3; }
        for (int dev = 0; dev < ndev && ctxs.size() < blocks.size(); ++dev) {
          bce_hip_ctx *c = nullptr;
          if (bce_hip_create(&c, dev) != 0) break;
          ctxs.push_back(c);
        }
      }
      const size_t workers = use_gpu ? ctxs.size() : std::min<size_t>(blocks.size(), 8);
      std::atomic<size_t> next_block{0};
      std::atomic<int> first_rc{0};
      // as in compress_blocks: a context that runs out of device memory (blocks of a GB and more, two contexts per device) gives
      // its memory back and leaves its block to ONE context that has the device to itself at the end
      std::vector<char> done(blocks.size(), 0);
      // a checked container: the CRC-32 of what block b decoded to -- on the device, from the decoder's own buffer, before the
      // text is copied back (-d), or of the bytes in the output (-ds) -- against the table's; a block that differs ends the run
      const int kMismatch = 1;                                      // (no bce_hip_status is positive)
      std::vector<uint32_t> got(blocks.size(), 0);
      std::vector<char> differs(blocks.size(), 0);
      auto decode_block = [&](bce_hip_ctx *c, size_t b) -> int {
        const uint8_t *ap = adata.data() + blocks[b].first;
        size_t n = 0;
        const size_t want = at[b + 1] - at[b];
        int r;
        if (c) r = checked ? bce_hip_decompress_device_crc32(c, ap, blocks[b].second, out.get() + at[b], want, &n, &got[b])
                           : bce_hip_decompress_device(c, ap, blocks[b].second, out.get() + at[b], want, &n);
        else {
          r = bce_hip_decompress(ap, blocks[b].second, out.get() + at[b], want, &n);
          if (r == 0 && checked && n == want) got[b] = bce_hip_crc32(0, out.get() + at[b], want);
        }
        if (r == 0 && n != want) r = BCE_HIP_E_INTERNAL;         // the table and the block's own header disagree
        if (r == 0 && checked && got[b] != table_crc(adata, b)) { differs[b] = 1; r = kMismatch; }
        return r;
      };
      std::vector<std::thread> th;
      for (size_t w = 0; w < workers; ++w)
        th.emplace_back([&, w] {
          while (first_rc.load() == 0) {
            const size_t b = next_block.fetch_add(1);
            if (b >= blocks.size()) break;
            bce_hip_ctx *c = use_gpu ? ctxs[w] : nullptr;
            const int r = decode_block(c, b);
            if (r == 0) { done[b] = 1; continue; }
            if (r == BCE_HIP_E_NOMEM && use_gpu) { bce_hip_destroy(ctxs[w]); ctxs[w] = nullptr; return; }   // (its block stays undone)
            int z = 0;
            first_rc.compare_exchange_strong(z, r);
          }
        });
      for (auto &t : th) t.join();
      rc = first_rc.load();
      for (bce_hip_ctx *&c : ctxs) { if (!c) continue; if (rc != 0 && bce_hip_last_error(c)[0]) printf("%s\n", bce_hip_last_error(c)); bce_hip_destroy(c); c = nullptr; }
      if (rc == 0 && use_gpu) {
        bce_hip_ctx *c = nullptr;
        for (size_t b = 0; rc == 0 && b < blocks.size(); ++b) {
          if (done[b]) continue;
          if (!c) rc = bce_hip_create(&c, 0);
          if (rc == 0) rc = decode_block(c, b);
          if (rc == 0) done[b] = 1;
        }
        if (rc != 0 && c && bce_hip_last_error(c)[0]) printf("%s\n", bce_hip_last_error(c));
        if (c) bce_hip_destroy(c);
      }
      if (rc == 0) for (size_t b = 0; b < blocks.size(); ++b) if (!done[b]) rc = BCE_HIP_E_INTERNAL;
      for (size_t b = 0; b < blocks.size(); ++b)
        if (differs[b]) {                                           // (the lowest block that differs; the file is not written)
          print_mismatch(b, table_crc(adata, b), got[b]);
          return -4;
        }
    }
    if (rc != 0) {
      printf("Decompression failed: %s\n", bce_hip_strerror(rc));
      if (rc == BCE_HIP_E_NOMEM && use_gpu) printf("(the GPU-assisted decoder holds 32 bytes of boundary ranks per input byte beside its node lists; `bce -ds` decodes on the host)\n");
      return -4;
    }
    auto end = std::chrono::high_resolution_clock::now();
    std::chrono::duration<double> duration = end - start;
    if (prefault.joinable()) prefault.join();
    if (!write_file(argv[2], out.get(), out_size)) { printf("Could not write file.\n"); if (keep) bce_hip_destroy(keep); return -5; }
    printf("Decompressed from %zu B -> %zu B in %.1f s\n", adata.size(), out_size, duration.count());
    lap("written");
    fast_exit(0);
    if (keep) bce_hip_destroy(keep);
    return 0;
  } else if (argc == 4 && argv[1][0] == '-' && argv[1][1] == 't' && argv[1][2] == 0) {
    return test_archive(argv[2], argv[3]);
  } else if (argc == 3 && argv[1][0] == '-' && argv[1][1] == 't' && argv[1][2] == 0) {
    return self_test_archive(argv[2]);
  } else if ((argc == 3 || argc == 4) && argv[1][0] == '-' && argv[1][1] == 'e' && argv[1][2] == 0) {
    return estimate_file(argv[2], argc == 4 ? argv[3] : nullptr);
  } else if (argc == 4 && argv[2][0] != 0 && (strcmp(argv[1], "-g") == 0 || strcmp(argv[1], "-gd") == 0)) {
    return count_command(argv[2], argv[3], argv[1][2] == 'd');
  } else if (argc == 4 && argv[2][0] != 0 && (strcmp(argv[1], "-gl") == 0 || strcmp(argv[1], "-gld") == 0)) {
    return locate_command(argv[2], argv[3], argv[1][3] == 'd');
  } else if (argc == 5 && argv[3][0] != 0 && (strcmp(argv[1], "-gn") == 0 || strcmp(argv[1], "-gnd") == 0) && parse_near_k(argv[2]) >= 0) {
    return count_near_command((uint32_t)parse_near_k(argv[2]), argv[3], argv[4], argv[1][3] == 'd');
  } else if (argc == 5 && argv[3][0] != 0 && (strcmp(argv[1], "-gw") == 0 || strcmp(argv[1], "-gwd") == 0) && parse_near_k(argv[2]) >= 0) {
    return count_edit_command((uint32_t)parse_near_k(argv[2]), argv[3], argv[4], argv[1][3] == 'd');
  } else if (argc == 5 && argv[3][0] != 0 && (strcmp(argv[1], "-gwl") == 0 || strcmp(argv[1], "-gwld") == 0) && parse_near_k(argv[2]) >= 0) {
    return locate_edit_command((uint32_t)parse_near_k(argv[2]), argv[3], argv[4], argv[1][4] == 'd');
  } else if (argc == 5 && argv[3][0] != 0 && (strcmp(argv[1], "-gnl") == 0 || strcmp(argv[1], "-gnld") == 0) && parse_near_k(argv[2]) >= 0) {
    return locate_near_command((uint32_t)parse_near_k(argv[2]), argv[3], argv[4], argv[1][4] == 'd');
  } else if (argc == 4 && argv[2][0] != 0 && strncmp(argv[1], "-ge", 3) == 0) {
    bool ignore_case = false, list = false, in_archive = false;
    std::vector<uint32_t> masks;
    if (!parse_class_option(argv[1], ignore_case, list, in_archive) ||
        !bce::compile_classes(reinterpret_cast<const uint8_t *>(argv[2]), strlen(argv[2]), ignore_case, masks) || masks.empty())
      return usage();
    return classes_command(masks, list, argv[3], in_archive);
  } else if (argc == 5 && (strcmp(argv[1], "-gm") == 0 || strcmp(argv[1], "-gmd") == 0) && parse_min_len(argv[2]) != 0) {
    return coverage_command(parse_min_len(argv[2]), argv[3], argv[1][3] == 'd', argv[4]);
  } else if (argc == 4 && (strcmp(argv[1], "-gz") == 0 || strcmp(argv[1], "-gzd") == 0) && parse_min_len(argv[2]) != 0) {
    return self_command(parse_min_len(argv[2]), argv[3], argv[1][3] == 'd');
  } else if (argc == 6 && (strcmp(argv[1], "-gr") == 0 || strcmp(argv[1], "-grd") == 0) && parse_min_len(argv[2]) != 0) {
    return delta_command(parse_min_len(argv[2]), argv[3], argv[1][3] == 'd', argv[4], argv[5]);
  } else if (argc == 5 && (strcmp(argv[1], "-ga") == 0 || strcmp(argv[1], "-gad") == 0)) {
    return apply_command(argv[2], argv[1][3] == 'd', argv[3], argv[4]);
  } else if (argc == 4 && (strcmp(argv[1], "-gk") == 0 || strcmp(argv[1], "-gkd") == 0) && parse_order(argv[2]) >= 0) {
    return kgrams_command((uint32_t)parse_order(argv[2]), argv[3], argv[1][3] == 'd');
  } else if (argc == 5 && (strcmp(argv[1], "-gf") == 0 || strcmp(argv[1], "-gfd") == 0) && parse_count(argv[2], kMaxTopLen) != 0 &&
             parse_count(argv[3], kMaxTopCount) != 0) {
    return top_command(parse_count(argv[2], kMaxTopLen), parse_count(argv[3], kMaxTopCount), argv[4], argv[1][3] == 'd');
  } else if (argc == 6 && (strcmp(argv[1], "-gp") == 0 || strcmp(argv[1], "-gpd") == 0) && parse_maxrep_order(argv[2]) >= 0 && parse_min_len(argv[3]) != 0 &&
             parse_count(argv[4], kMaxTopCount) != 0) {
    return maxrep_command((uint32_t)parse_maxrep_order(argv[2]), parse_min_len(argv[3]), parse_count(argv[4], kMaxTopCount), argv[5], argv[1][3] == 'd');
  } else if (argc == 4 && (strcmp(argv[1], "-gs") == 0 || strcmp(argv[1], "-gsd") == 0)) {
    return sa_command(argv[2], argv[1][3] == 'd', argv[3]);
  } else if (argc == 4 && strcmp(argv[1], "-gsc") == 0) {
    return sa_check_command(argv[2], argv[3]);
  } else if (argc == 4 && argv[1][0] == '-' && argv[1][1] == 's') {
    // Scan (bce.cpp:1384-1402): enumeration on the GPU, ScanCoder optimisation on the host, 288-byte config out
    auto start = std::chrono::high_resolution_clock::now();
    HostFile data;
    std::thread reader(read_whole_file, argv[3], &data, kMaxInput);
    bce_hip_ctx *ctx = nullptr;
    int rc = bce_hip_create(&ctx, 0);
    reader.join();
    if (rc != 0) { printf("No usable HIP device: %s\n", bce_hip_strerror(rc)); return -3; }
    if (data.status != 0 || data.size() == 0 || data.size() >= kMaxInput) { printf("Error loading file\n"); bce_hip_destroy(ctx); return -1; }
    uint8_t cfg[BCE_HIP_CONFIG_BYTES];
    double res[9];
    rc = bce_hip_load_host(ctx, data.data(), (uint32_t)data.size());
    if (rc == 0) rc = bce_hip_bwt(ctx, nullptr);
    if (rc == 0) rc = bce_hip_build_planes(ctx, nullptr);
    uint64_t prog = 0;
    bce_hip_set_progress(ctx, progress, &prog);
    if (rc == 0) rc = bce_hip_scan(ctx, cfg, res);
    progress_end();
    if (rc != 0) { printf("Scan failed: %s (%s)\n", bce_hip_strerror(rc), bce_hip_last_error(ctx)); bce_hip_destroy(ctx); return -4; }
    for (int i = 0; i < 9; ++i) printf("Result size: %.1f B\n", res[i]);            // ScanCoder::flush, :799
    if (!write_file(argv[2], cfg, BCE_HIP_CONFIG_BYTES)) { printf("Could not write Config.\n"); bce_hip_destroy(ctx); return -5; }   // save_config, :810-813
    auto end = std::chrono::high_resolution_clock::now();
    std::chrono::duration<double> duration = end - start;
    printf("Scanned %zu B in %.1f s\n", data.size(), duration.count());
    fast_exit(0);
    bce_hip_destroy(ctx);
    return 0;
  }
  return usage();
}
