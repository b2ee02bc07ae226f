// Near-duplicate detection: token hashes, MinHash signatures and an exact band index, on the device.
//
// Replaces the arithmetic of reference buglab/data/deduplication/index.py:32-46 (`check_if_duplicate_and_add`: a 256-permutation
// MinHash updated one token at a time in NumPy, then a look-up and an insert in one Python dict per LSH band) -- restated from
// the MinHash / MinHash-LSH definition the reference delegates to and frozen in DESIGN.md ("Near-duplicate detection").  All of it
// is integer arithmetic, so every result is checked bit for bit (tests/test_dedup_gpu.py against tests/dedup_ref.py).
//
//   dedup_sha1_kernel     one thread per token: SHA-1 of the token's UTF-8 bytes (any length: a 64-byte block at a time, the
//                         padding generated on the fly), hv = the first four digest bytes read as a little-endian uint32.
//   dedup_minhash_kernel  one workgroup per document, one permutation per lane (a, b in registers); the document's token hashes
//                         go through LDS DD_CHUNK at a time, every lane reading the same word (a broadcast), so a document of
//                         any length needs 4 KB of LDS.  sig[k] = min over tokens of ((a[k] hv + b[k]) mod 2^64) mod (2^61 - 1),
//                         low 32 bits; the Mersenne reduction is (x & M) + (x >> 61) and one conditional subtract.
//   dedup_lsh_insert_kernel / dedup_lsh_query_kernel
//                         the band index: per band one open-addressing table (linear probing) of document numbers.  A slot
//                         belongs to ONE band key for good -- the key of the document that claimed it with compare-and-swap --
//                         and holds the smallest number inserted with that key (atomic minimum).  A key is recognised by
//                         comparing all `rows` signature values with those of the document in the slot, never by its hash, so
//                         the index is exact.  Which slot a key gets depends on the order of arrival; what the slot ends up
//                         holding does not, and the query runs as a second launch after every insert has landed: document i is
//                         a duplicate iff, in some band, the smallest number filed under its key is below i.  That is the answer
//                         of inserting the documents one at a time in number order, for every batch split.
#include "bl_common.h"
#include "bl_segment_f64.h"  // bl_clamp_off

namespace {
constexpr int DD_THREADS = 256;
constexpr int DD_CHUNK = 1024;  // token hashes staged in LDS per pass
constexpr uint32_t DD_EMPTY = 0xFFFFFFFFu;
constexpr uint64_t DD_MERSENNE = (1ull << 61) - 1;

__device__ __forceinline__ uint32_t dd_rotl(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }

// byte i of the padded message: the token, 0x80, zeros, the bit length as a big-endian uint64 in the last 8 bytes
__device__ __forceinline__ uint32_t dd_padded_byte(const uint8_t* __restrict__ msg, int64_t len, int64_t total, int64_t i) {
  if (i < len) return msg[i];
  if (i == len) return 0x80u;
  if (i < total - 8) return 0u;
  const uint64_t bits = (uint64_t)len * 8u;
  return (uint32_t)(bits >> (8 * (total - 1 - i))) & 0xFFu;
}

__global__ __launch_bounds__(DD_THREADS) void dedup_sha1_kernel(const uint8_t* __restrict__ bytes, int64_t nbytes,
                                                                const int64_t* __restrict__ tok_off, int64_t ntokens,
                                                                uint32_t* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * DD_THREADS + threadIdx.x;
  if (t >= ntokens) return;
  const int64_t o0 = bl_clamp_off(tok_off[t], nbytes), o1 = bl_clamp_off(tok_off[t + 1], nbytes);
  const int64_t len = o1 > o0 ? o1 - o0 : 0;
  const uint8_t* msg = bytes + o0;
  const int64_t total = (len + 9 + 63) / 64 * 64;  // 56 bytes and more need a second block, 120 and more a third
  uint32_t h0 = 0x67452301u, h1 = 0xEFCDAB89u, h2 = 0x98BADCFEu, h3 = 0x10325476u, h4 = 0xC3D2E1F0u;
  for (int64_t blk = 0; blk < total; blk += 64) {
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int64_t p = blk + 4 * i;
      uint32_t v;
      if (p + 4 <= len)
        v = ((uint32_t)msg[p] << 24) | ((uint32_t)msg[p + 1] << 16) | ((uint32_t)msg[p + 2] << 8) | (uint32_t)msg[p + 3];
      else
        v = (dd_padded_byte(msg, len, total, p) << 24) | (dd_padded_byte(msg, len, total, p + 1) << 16) |
            (dd_padded_byte(msg, len, total, p + 2) << 8) | dd_padded_byte(msg, len, total, p + 3);
      w[i] = v;
    }
    uint32_t a = h0, b = h1, c = h2, d = h3, e = h4;
#pragma unroll
    for (int i = 0; i < 80; ++i) {
      if (i >= 16) w[i & 15] = dd_rotl(w[(i + 13) & 15] ^ w[(i + 8) & 15] ^ w[(i + 2) & 15] ^ w[i & 15], 1);
      uint32_t f, k;
      if (i < 20) {
        f = (b & c) | (~b & d);
        k = 0x5A827999u;
      } else if (i < 40) {
        f = b ^ c ^ d;
        k = 0x6ED9EBA1u;
      } else if (i < 60) {
        f = (b & c) | (b & d) | (c & d);
        k = 0x8F1BBCDCu;
      } else {
        f = b ^ c ^ d;
        k = 0xCA62C1D6u;
      }
      const uint32_t tmp = dd_rotl(a, 5) + f + e + k + w[i & 15];
      e = d;
      d = c;
      c = dd_rotl(b, 30);
      b = a;
      a = tmp;
    }
    h0 += a;
    h1 += b;
    h2 += c;
    h3 += d;
    h4 += e;
  }
  // the digest starts with h0 big-endian; its first four bytes as a little-endian integer = h0 byte-swapped
  out[t] = __builtin_bswap32(h0);
}

__global__ __launch_bounds__(DD_THREADS) void dedup_minhash_kernel(const uint32_t* __restrict__ hashes, int64_t nhashes,
                                                                   const int64_t* __restrict__ doc_off,
                                                                   const uint64_t* __restrict__ perm_a,
                                                                   const uint64_t* __restrict__ perm_b, int num_perm,
                                                                   uint32_t* __restrict__ sigs) {
  __shared__ uint32_t s_hv[DD_CHUNK];
  const int64_t doc = blockIdx.x;
  const int k = threadIdx.x;
  const bool live = k < num_perm;
  const uint64_t a = live ? perm_a[k] : 1u, b = live ? perm_b[k] : 0u;
  const int64_t t0 = bl_clamp_off(doc_off[doc], nhashes), t1 = bl_clamp_off(doc_off[doc + 1], nhashes);
  uint32_t best = 0xFFFFFFFFu;
  for (int64_t base = t0; base < t1; base += DD_CHUNK) {
    const int n = (int)(t1 - base < DD_CHUNK ? t1 - base : DD_CHUNK);
    __syncthreads();  // the previous chunk has been read by every lane
    for (int i = threadIdx.x; i < n; i += blockDim.x) s_hv[i] = hashes[base + i];
    __syncthreads();
    for (int i = 0; i < n; ++i) {
      const uint64_t x = a * (uint64_t)s_hv[i] + b;  // wraps at 64 bits: part of the specification
      uint64_t y = (x & DD_MERSENNE) + (x >> 61);    // <= M + 7
      if (y >= DD_MERSENNE) y -= DD_MERSENNE;
      const uint32_t v = (uint32_t)y;
      best = v < best ? v : best;
    }
  }
  if (live) sigs[doc * num_perm + k] = best;
}

// where a band key starts probing; never used to tell two keys apart
__device__ __forceinline__ uint32_t dd_band_hash(const uint32_t* __restrict__ band, int rows) {
  uint32_t h = 0x9E3779B9u;
  for (int i = 0; i < rows; ++i) h = bl_lowbias32(h ^ band[i]) + 0x7F4A7C15u;
  return h;
}
__device__ __forceinline__ bool dd_band_equal(const uint32_t* __restrict__ x, const uint32_t* __restrict__ y, int rows) {
  bool eq = true;
  for (int i = 0; i < rows; ++i) eq = eq && x[i] == y[i];
  return eq;
}

__global__ __launch_bounds__(DD_THREADS) void dedup_lsh_insert_kernel(const uint32_t* __restrict__ sigs, int num_perm, int bands,
                                                                      int rows, uint32_t* __restrict__ table, int64_t slots,
                                                                      int64_t first, int64_t count, int32_t* __restrict__ status) {
  const int64_t w = (int64_t)blockIdx.x * DD_THREADS + threadIdx.x;
  if (w >= count * bands) return;
  const int64_t id = first + w / bands;
  const int band = (int)(w % bands);
  const uint32_t* mine = sigs + id * num_perm + band * rows;
  uint32_t* tab = table + (int64_t)band * slots;
  int64_t s = dd_band_hash(mine, rows) & (uint64_t)(slots - 1);
  for (int64_t probe = 0; probe < slots; ++probe, s = (s + 1) & (slots - 1)) {
    const uint32_t old = atomicCAS(&tab[s], DD_EMPTY, (uint32_t)id);
    if (old == DD_EMPTY) return;  // claimed for this key
    if ((int64_t)old < first + count && dd_band_equal(mine, sigs + (int64_t)old * num_perm + band * rows, rows)) {
      atomicMin(&tab[s], (uint32_t)id);
      return;
    }
  }
  atomicOr(status, 1);  // no free slot: the caller broke the load bound
}

__global__ __launch_bounds__(DD_THREADS) void dedup_lsh_query_kernel(const uint32_t* __restrict__ sigs, int num_perm, int bands,
                                                                     int rows, const uint32_t* __restrict__ table, int64_t slots,
                                                                     int64_t first, int64_t count, int64_t total,
                                                                     int32_t* __restrict__ flags, int32_t* __restrict__ status) {
  const int64_t w = (int64_t)blockIdx.x * DD_THREADS + threadIdx.x;
  if (w >= count * bands) return;
  const int64_t id = first + w / bands;
  const int band = (int)(w % bands);
  const uint32_t* mine = sigs + id * num_perm + band * rows;
  const uint32_t* tab = table + (int64_t)band * slots;
  int64_t s = dd_band_hash(mine, rows) & (uint64_t)(slots - 1);
  for (int64_t probe = 0; probe < slots; ++probe, s = (s + 1) & (slots - 1)) {
    const uint32_t cur = tab[s];
    if (cur == DD_EMPTY) break;  // the document was never inserted
    if ((int64_t)cur < total && dd_band_equal(mine, sigs + (int64_t)cur * num_perm + band * rows, rows)) {
      if ((int64_t)cur < id) atomicOr(&flags[id - first], 1);
      return;
    }
  }
  atomicOr(status, 2);
}
}  // namespace

extern "C" int bl_dedup_sha1_u32(const uint8_t* bytes, int64_t nbytes, const int64_t* tok_off, int64_t ntokens, uint32_t* out,
                                 void* stream) {
  BL_CHECK_ARG(nbytes >= 0 && ntokens >= 0, "bl_dedup_sha1_u32: negative size (nbytes %lld, ntokens %lld)", (long long)nbytes,
               (long long)ntokens);
  BL_CHECK_ARG(ntokens == 0 || (tok_off && out), "bl_dedup_sha1_u32: null tok_off / out");
  BL_CHECK_ARG(nbytes == 0 || bytes, "bl_dedup_sha1_u32: null bytes with nbytes %lld", (long long)nbytes);
  const int64_t blocks = (ntokens + DD_THREADS - 1) / DD_THREADS;
  BL_CHECK_RANGE(bl_fits_int32(blocks), "bl_dedup_sha1_u32: %lld tokens in one call, at most %lld", (long long)ntokens,
                 (long long)0x7fffffff * DD_THREADS);
  if (ntokens == 0) return BL_OK;
  hipLaunchKernelGGL(dedup_sha1_kernel, dim3((unsigned)blocks), dim3(DD_THREADS), 0, (hipStream_t)stream, bytes, nbytes, tok_off,
                     ntokens, out);
  BL_LAUNCH_CHECK("bl_dedup_sha1_u32");
  return BL_OK;
}

extern "C" int bl_dedup_minhash(const uint32_t* hashes, int64_t nhashes, const int64_t* doc_off, int64_t ndocs, const uint64_t* perm_a,
                                const uint64_t* perm_b, int32_t num_perm, uint32_t* sigs, void* stream) {
  BL_CHECK_ARG(num_perm >= 1 && num_perm <= BL_DEDUP_MAX_PERM,
               "bl_dedup_minhash: num_perm = %d, the kernel covers 1 .. %d (one permutation per lane of one workgroup)", (int)num_perm,
               BL_DEDUP_MAX_PERM);
  BL_CHECK_ARG(nhashes >= 0 && ndocs >= 0, "bl_dedup_minhash: negative size (nhashes %lld, ndocs %lld)", (long long)nhashes,
               (long long)ndocs);
  BL_CHECK_ARG(ndocs == 0 || (doc_off && perm_a && perm_b && sigs), "bl_dedup_minhash: null doc_off / perm_a / perm_b / sigs");
  BL_CHECK_ARG(nhashes == 0 || hashes, "bl_dedup_minhash: null hashes with nhashes %lld", (long long)nhashes);
  BL_CHECK_RANGE(bl_fits_int32(ndocs), "bl_dedup_minhash: %lld documents in one call, at most %d", (long long)ndocs, 0x7fffffff);
  if (ndocs == 0) return BL_OK;
  const int threads = (num_perm + BL_WAVE - 1) / BL_WAVE * BL_WAVE;
  hipLaunchKernelGGL(dedup_minhash_kernel, dim3((unsigned)ndocs), dim3(threads), 0, (hipStream_t)stream, hashes, nhashes, doc_off, perm_a,
                     perm_b, (int)num_perm, sigs);
  BL_LAUNCH_CHECK("bl_dedup_minhash");
  return BL_OK;
}

extern "C" int bl_dedup_lsh_insert_query(const uint32_t* sigs, int32_t num_perm, int32_t bands, int32_t rows, uint32_t* table,
                                         int64_t slots, int64_t insert_from, int64_t query_from, int64_t total, int32_t* flags,
                                         int32_t* status, void* stream) {
  BL_CHECK_ARG(num_perm >= 1 && num_perm <= BL_DEDUP_MAX_PERM, "bl_dedup_lsh_insert_query: num_perm = %d, the kernels cover 1 .. %d",
               (int)num_perm, BL_DEDUP_MAX_PERM);
  BL_CHECK_ARG(bands >= 1 && rows >= 1 && (int64_t)bands * rows <= num_perm,
               "bl_dedup_lsh_insert_query: bands x rows = %d x %d does not fit num_perm = %d", (int)bands, (int)rows, (int)num_perm);
  BL_CHECK_ARG(slots >= 2 && (slots & (slots - 1)) == 0, "bl_dedup_lsh_insert_query: slots = %lld, need a power of two >= 2",
               (long long)slots);
  BL_CHECK_ARG(insert_from >= 0 && insert_from <= total && query_from >= 0 && query_from <= total,
               "bl_dedup_lsh_insert_query: need 0 <= insert_from (%lld), query_from (%lld) <= total (%lld)", (long long)insert_from,
               (long long)query_from, (long long)total);
  BL_CHECK_ARG(2 * total <= slots,
               "bl_dedup_lsh_insert_query: %lld documents in %lld slots per band: the load bound is 1/2, rebuild at a larger capacity",
               (long long)total, (long long)slots);
  BL_CHECK_ARG(total == 0 || (sigs && table && status), "bl_dedup_lsh_insert_query: null sigs / table / status");
  BL_CHECK_ARG(query_from == total || flags, "bl_dedup_lsh_insert_query: null flags with %lld documents to answer for",
               (long long)(total - query_from));
  const int64_t nins = (total - insert_from) * bands, nq = (total - query_from) * bands;
  const int64_t bins = (nins + DD_THREADS - 1) / DD_THREADS, bq = (nq + DD_THREADS - 1) / DD_THREADS;
  BL_CHECK_RANGE(total < 0x7fffffff && bl_fits_int32(bins) && bl_fits_int32(bq),
                 "bl_dedup_lsh_insert_query: %lld documents: document numbers and launch sizes are 31-bit", (long long)total);
  if (bins > 0) {
    hipLaunchKernelGGL(dedup_lsh_insert_kernel, dim3((unsigned)bins), dim3(DD_THREADS), 0, (hipStream_t)stream, sigs, (int)num_perm,
                       (int)bands, (int)rows, table, slots, insert_from, total - insert_from, status);
    BL_LAUNCH_CHECK("bl_dedup_lsh_insert_query (insert)");
  }
  if (bq > 0) {
    const hipError_t e = hipMemsetAsync(flags, 0, sizeof(int32_t) * (size_t)(total - query_from), (hipStream_t)stream);
    if (e != hipSuccess) {
      bl_set_error("bl_dedup_lsh_insert_query: clearing the flags failed: %s", hipGetErrorString(e));
      return (int)e;
    }
    hipLaunchKernelGGL(dedup_lsh_query_kernel, dim3((unsigned)bq), dim3(DD_THREADS), 0, (hipStream_t)stream, sigs, (int)num_perm,
                       (int)bands, (int)rows, table, slots, query_from, total - query_from, total, flags, status);
    BL_LAUNCH_CHECK("bl_dedup_lsh_insert_query (query)");
  }
  return BL_OK;
}
