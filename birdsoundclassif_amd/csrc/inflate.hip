// DEFLATE on the device (RFC 1950 / 1951): the IDAT payloads of a batch of PNG files -> the filtered scanlines that
// `nbm_png_unfilter_gray8` (dataset.hip) takes.  Replaces the zlib half of `imageio.imread` (reference
// nbm_datasets/image_dataset.py:44,62,77) that `Img_dataset.raw_item` otherwise runs on the host.
//
// One wavefront per stream (a batch is 256-320 streams on 256 CUs: latency per symbol, not occupancy, sets the time).
// The symbol loop is wave-uniform: every lane carries the same bit buffer and position, table entries come out of LDS
// through readfirstlane so that the state lives in scalar registers.  The 64 lanes work in parallel where there is
// something to share out: staging the payload (16 bytes per lane into a 1 KiB LDS chunk, the bit buffer refills from
// there 4 aligned bytes at a time), match and stored-block copies, building the decode tables (a ballot per code length
// ranks the symbols, then one canonical decode per fast-table entry), flushing the window (16-byte stores) and the
// Adler-32 of what is flushed.
//
// The 32 KiB window is a ring in LDS: a back-reference never reads global memory.  Whenever 1 KiB of new output stands
// in the ring it is stored to `out` and summed, so at most 1 KiB + one symbol is ever unflushed and nothing that a
// distance <= 32 768 can reach has been overwritten.
//
// Safety: every payload read is below the stream's length (bytes past it read as zero and using one ends the stream
// with NBM_INFLATE_EINPUT), every output write is below `expect`, every loop iteration consumes at least one input bit
// or is counted by a bound known beforehand, so the work is bounded by expect + 8 * length.  No atomics; the status of
// every stream is written unconditionally.
#include "nbm_common.h"

namespace {

constexpr int RING = 32768, RMASK = RING - 1;
constexpr int IN_CHUNK = 1024;                    // payload bytes staged in LDS at a time
constexpr int FLUSH = 1024;                       // output bytes per flush: 64 lanes x 16
constexpr int LIT_BITS = 10, DIST_BITS = 8, CL_BITS = 7;
constexpr int MAX_LENS = 320;                     // 288 + 32 (fixed block) >= 286 + 30 (dynamic block)

struct __attribute__((aligned(16))) InflateLds {
  uint8_t ring[RING];
  uint32_t in[IN_CHUNK / 4];
  uint16_t litfast[1 << LIT_BITS];                // (symbol << 4) | code length; 0: longer than the index or unassigned
  uint16_t distfast[1 << DIST_BITS];
  uint16_t clfast[1 << CL_BITS];
  uint16_t litsym[288], distsym[32], clsym[32];   // symbols in canonical order
  uint16_t litcnt[16], distcnt[16], clcnt[16];    // codes per length
  uint8_t lens[MAX_LENS];
  uint8_t cllens[32];
};

__device__ __forceinline__ uint32_t rfl(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// Canonical Huffman decode of the code that starts at bit 0 of `bits` (first bit of the stream = most significant bit
// of the code), at most `maxlen` bits long: (symbol << 4) | length, or 0 when no code of that length matches.
// index + (code - first) < sum of cnt: always inside symtab.
__device__ __forceinline__ uint32_t canon_decode(uint32_t bits, const uint16_t* cnt, const uint16_t* symtab, int maxlen) {
  int code = 0, first = 0, index = 0;
  for (int l = 1; l <= maxlen; ++l) {
    code |= (int)(bits & 1u);
    bits >>= 1;
    const int c = cnt[l];
    if (code - c < first) return ((uint32_t)symtab[index + (code - first)] << 4) | (uint32_t)l;
    index += c;
    first = (first + c) * 2;
    code *= 2;
  }
  return 0;
}

struct CodeSet {
  int left;      // 0: complete, > 0: incomplete, < 0: over-subscribed (zlib's `left`)
  int maxlen;    // longest code length in use, 0: no code at all
};

// lens[0 .. n) (n <= 320, lengths 0..15) -> cnt, symtab and the fast table of 2^fbits entries.  One copy of the code
// for the five call sites.  The lane-strided loops of this file are marked vectorize(disable): the loop vectoriser has
// nothing to gain on them, and its predicated stores once left a wave's exec mask empty.
__device__ __noinline__ CodeSet build_tables(const uint8_t* lens, int n, uint16_t* cnt, uint16_t* symtab, uint16_t* fast, int fbits,
                                int lane) {
  __syncthreads();                                 // lens written by other lanes; earlier readers of the tables are done
  int l[5];
#pragma unroll
  for (int b = 0; b < 5; ++b) l[b] = (b * 64 + lane < n) ? lens[b * 64 + lane] : 0;
  const unsigned long long below = (1ull << lane) - 1ull;
  int off = 0;
  CodeSet cs{1, 0};
  for (int L = 1; L <= 15; ++L) {
    const int start = off;
#pragma unroll
    for (int b = 0; b < 5; ++b) {
      const unsigned long long m = __ballot(l[b] == L);
      if (l[b] == L) symtab[off + __popcll(m & below)] = (uint16_t)(b * 64 + lane);     // off + rank < n <= table size
      off += __popcll(m);
    }
    const int c = off - start;
    if (lane == 0) cnt[L] = (uint16_t)c;
    cs.left = cs.left * 2 - c;                     // >= -320 * 2^15: no overflow
    if (c) cs.maxlen = L;
  }
  __syncthreads();
#pragma clang loop vectorize(disable) interleave(disable)
  for (int e = lane; e < (1 << fbits); e += 64) fast[e] = (uint16_t)canon_decode((uint32_t)e, cnt, symtab, fbits);
  __syncthreads();
  return cs;
}

struct Inflater {
  InflateLds& s;
  const uint8_t* src;       // the stream, 16-byte aligned
  uint32_t len;             // its length in bytes
  uint8_t* row;             // output row, 16-byte aligned
  uint32_t expect;
  int lane;
  // bit reader (wave-uniform)
  uint64_t buf = 0;
  uint32_t cnt = 0;         // valid bits in buf
  uint32_t w = 0;           // next 4-byte word of the stream to fetch
  uint32_t chunk = 0xFFFFFFFFu;   // index of the 1 KiB chunk staged in s.in
  // output (wave-uniform)
  uint32_t pos = 0, flushed = 0;
  uint32_t adler_a = 1, adler_b = 0;

  __device__ Inflater(InflateLds& s_, const uint8_t* src_, uint32_t len_, uint8_t* row_, uint32_t expect_, int lane_)
      : s(s_), src(src_), len(len_), row(row_), expect(expect_), lane(lane_) {}

  __device__ void stage(uint32_t c) {
    const uint32_t o = c * IN_CHUNK + lane * 16;            // len <= 2^30: no overflow
    uint4 v = make_uint4(0, 0, 0, 0);
    if (o + 16 <= len) {
      v = *reinterpret_cast<const uint4*>(src + o);
    } else if (o < len) {                                   // the stream's last bytes, one at a time: never past len
      uint32_t t[4] = {0, 0, 0, 0};
      for (uint32_t j = 0; j < 16 && o + j < len; ++j) t[j >> 2] |= (uint32_t)src[o + j] << (8 * (j & 3));
      v = make_uint4(t[0], t[1], t[2], t[3]);
    }
    __syncthreads();
    reinterpret_cast<uint4*>(s.in)[lane] = v;
    __syncthreads();
    chunk = c;
  }

  // afterwards cnt >= 32
  __device__ __forceinline__ void need32() {
    if (cnt <= 32) {
      if ((w >> 8) != chunk) stage(w >> 8);
      const uint32_t x = rfl(s.in[w & 255u]);
      buf |= (uint64_t)x << cnt;
      cnt += 32;
      ++w;
    }
  }
  __device__ __forceinline__ uint32_t peek(uint32_t n) const { return (uint32_t)buf & ((1u << n) - 1u); }
  __device__ __forceinline__ void drop(uint32_t n) { buf >>= n; cnt -= n; }
  // a bit past the end of the stream has been consumed
  __device__ __forceinline__ bool exhausted() const { return w * 4u - (cnt >> 3) > len; }
  __device__ __forceinline__ int fail(int code) const { return exhausted() ? NBM_INFLATE_EINPUT : code; }

  // store ring bytes [flushed, flushed + n), n <= 1024, to the row and take them into the Adler-32 sums
  __device__ void flush(uint32_t n) {
    __syncthreads();
    const uint32_t o = (uint32_t)lane * 16u;
    const uint4 v = *reinterpret_cast<const uint4*>(s.ring + ((flushed + o) & RMASK));    // flushed % 1024 == 0
    const uint32_t q[4] = {v.x, v.y, v.z, v.w};
    uint32_t s1 = 0, s2 = 0;
#pragma unroll
    for (uint32_t j = 0; j < 16; ++j) {
      const uint32_t d = (o + j < n) ? ((q[j >> 2] >> (8 * (j & 3))) & 0xFFu) : 0u;
      s1 += d;
      s2 += d * (n - (o + j));                     // 0 where d is masked; <= 1024 * 255 per byte
    }
    if (o + 16 <= n) {
      *reinterpret_cast<uint4*>(row + flushed + o) = v;                                    // flushed + n <= expect
    } else {
      for (uint32_t j = 0; j < 16 && o + j < n; ++j) row[flushed + o + j] = (uint8_t)(q[j >> 2] >> (8 * (j & 3)));
    }
#pragma unroll
    for (int x = 32; x > 0; x >>= 1) {
      s1 += (uint32_t)__shfl_xor((int)s1, x);
      s2 += (uint32_t)__shfl_xor((int)s2, x);      // <= 255 * 1024 * 1025 / 2 < 2^28
    }
    s1 = rfl(s1), s2 = rfl(s2);
    adler_b = (adler_b + n * adler_a + s2) % 65521u;                                       // < 2^16 + 2^26 + 2^28
    adler_a = (adler_a + s1) % 65521u;
    flushed += n;
  }

  __device__ int stored_block() {
    drop(cnt & 7u);
    need32();
    const uint32_t n = peek(16), nn = (uint32_t)(buf >> 16) & 0xFFFFu;
    drop(32);
    if (exhausted()) return NBM_INFLATE_EINPUT;
    if ((n ^ 0xFFFFu) != nn) return NBM_INFLATE_ESTORED;
    uint32_t at = w * 4u - (cnt >> 3);                      // byte position of the block's data (cnt % 8 == 0)
    if (at + n > len) return NBM_INFLATE_EINPUT;
    if (n > expect - pos) return NBM_INFLATE_EOUTPUT;
    for (uint32_t j = 0; j < n; j += 256) {
      const uint32_t m = n - j < 256u ? n - j : 256u;
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t i = k * 64 + lane;
        if (i < m) s.ring[(pos + i) & RMASK] = src[at + j + i];                            // at + j + i < at + n <= len
      }
      pos += m;
      if (pos - flushed >= FLUSH) flush(FLUSH);
    }
    at += n;
    buf = 0, cnt = 0, w = at >> 2;                          // go on behind the data: refill from its word, drop its head
    need32();
    drop(8u * (at & 3u));
    return NBM_OK;
  }

  __device__ int fixed_tables() {
    __syncthreads();
#pragma unroll
    for (int b = 0; b < MAX_LENS / 64; ++b) {               // 320 = 5 x 64: every lane stores five lengths, no guard
      const int i = b * 64 + lane;
      s.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
    }
    build_tables(s.lens, 288, s.litcnt, s.litsym, s.litfast, LIT_BITS, lane);
    build_tables(s.lens + 288, 32, s.distcnt, s.distsym, s.distfast, DIST_BITS, lane);     // 30 and 31: refused when met
    return NBM_OK;
  }

  __device__ int dynamic_tables() {
    need32();
    const uint32_t hlit = peek(5) + 257u, hdist = ((uint32_t)(buf >> 5) & 31u) + 1u, hclen = ((uint32_t)(buf >> 10) & 15u) + 4u;
    drop(14);
    if (exhausted()) return NBM_INFLATE_EINPUT;
    if (hlit > 286u || hdist > 30u) return NBM_INFLATE_ECODELENGTHS;
    __syncthreads();
    if (lane < 32) s.cllens[lane] = 0;
    __syncthreads();
    for (uint32_t i = 0; i < hclen; ++i) {
      // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, five bits each
      const uint32_t o = i < 12 ? (uint32_t)(0x22CAA324E804A30ull >> (5 * i)) & 31u
                                : (uint32_t)(0x3C2E1346Cull >> (5 * (i - 12))) & 31u;
      need32();
      if (lane == 0) s.cllens[o] = (uint8_t)peek(3);
      drop(3);
    }
    if (exhausted()) return NBM_INFLATE_EINPUT;
    CodeSet cs = build_tables(s.cllens, 19, s.clcnt, s.clsym, s.clfast, CL_BITS, lane);
    if (cs.left != 0) return NBM_INFLATE_ECODESET;
    const uint32_t total = hlit + hdist;
    uint32_t i = 0, prev = 0;
    while (i < total) {                                     // every turn adds at least one length: <= 316 turns
      need32();
      const uint32_t e = rfl(s.clfast[peek(CL_BITS)]);
      if (!e) return fail(NBM_INFLATE_ECODESET);            // cannot happen with a complete set of <= 7-bit codes
      drop(e & 15u);
      const uint32_t sym = e >> 4;
      if (sym < 16u) {
        if (lane == 0) s.lens[i] = (uint8_t)sym;
        prev = sym;
        ++i;
      } else {
        uint32_t rep, val = 0;
        if (sym == 16u) {
          if (i == 0) return fail(NBM_INFLATE_ECODELENGTHS);
          val = prev, rep = 3u + peek(2), drop(2);
        } else if (sym == 17u) {
          rep = 3u + peek(3), drop(3);
        } else {
          rep = 11u + peek(7), drop(7);
        }
        if (i + rep > total) return fail(NBM_INFLATE_ECODELENGTHS);
#pragma clang loop vectorize(disable) interleave(disable)
        for (uint32_t k = lane; k < rep; k += 64) s.lens[i + k] = (uint8_t)val;            // i + k < total <= 316
        i += rep, prev = val;
      }
      if (exhausted()) return NBM_INFLATE_EINPUT;
    }
    __syncthreads();
    if (rfl(s.lens[256]) == 0) return NBM_INFLATE_ECODELENGTHS;                            // no end-of-block code
    cs = build_tables(s.lens, (int)hlit, s.litcnt, s.litsym, s.litfast, LIT_BITS, lane);
    if (cs.left < 0 || (cs.left > 0 && cs.maxlen != 1)) return NBM_INFLATE_ECODESET;       // zlib inftrees.c's rule
    cs = build_tables(s.lens + hlit, (int)hdist, s.distcnt, s.distsym, s.distfast, DIST_BITS, lane);
    if (cs.left < 0 || (cs.left > 0 && cs.maxlen > 1)) return NBM_INFLATE_ECODESET;
    return NBM_OK;
  }

  __device__ int coded_block() {
    for (;;) {                                              // every turn consumes at least one bit
      need32();
      uint32_t e = rfl(s.litfast[peek(LIT_BITS)]);
      if ((e & 15u) == 0) {
        e = rfl(canon_decode(peek(15), s.litcnt, s.litsym, 15));
        if (!e) return fail(NBM_INFLATE_ECODE);
      }
      drop(e & 15u);
      uint32_t sym = e >> 4;
      if (exhausted()) return NBM_INFLATE_EINPUT;
      if (sym < 256u) {
        if (pos >= expect) return NBM_INFLATE_EOUTPUT;
        if (lane == 0) s.ring[pos & RMASK] = (uint8_t)sym;
        ++pos;
      } else if (sym == 256u) {
        return NBM_OK;
      } else {
        sym -= 257u;
        if (sym >= 29u) return NBM_INFLATE_ECODE;
        uint32_t n;
        if (sym < 8u) {
          n = 3u + sym;
        } else if (sym == 28u) {
          n = 258u;
        } else {
          const uint32_t x = (sym - 4u) >> 2;
          n = 3u + ((4u + (sym & 3u)) << x) + peek(x);
          drop(x);
        }
        need32();
        e = rfl(s.distfast[peek(DIST_BITS)]);
        if ((e & 15u) == 0) {
          e = rfl(canon_decode(peek(15), s.distcnt, s.distsym, 15));
          if (!e) return fail(NBM_INFLATE_ECODE);
        }
        drop(e & 15u);
        const uint32_t ds = e >> 4;
        if (ds >= 30u) return fail(NBM_INFLATE_ECODE);
        uint32_t dist;
        if (ds < 4u) {
          dist = 1u + ds;
        } else {
          const uint32_t x = (ds - 2u) >> 1;
          dist = 1u + ((2u + (ds & 1u)) << x) + peek(x);
          drop(x);
        }
        if (exhausted()) return NBM_INFLATE_EINPUT;
        if (dist > pos) return NBM_INFLATE_EDISTANCE;
        if (n > expect - pos) return NBM_INFLATE_EOUTPUT;
        // byte i of the match = byte (i mod dist) of the dist bytes in front of it: every source byte was written
        // before this match, whatever the overlap; a source and a destination slot coincide only at dist == 32 768,
        // where the lane that reads the slot is the one that rewrites it
        const uint32_t from = pos - dist;
        __syncthreads();
        if (dist >= n) {
#pragma clang loop vectorize(disable) interleave(disable)
          for (uint32_t i = lane; i < n; i += 64) {
            const uint8_t b = s.ring[(from + i) & RMASK];
            s.ring[(pos + i) & RMASK] = b;
          }
        } else {
#pragma clang loop vectorize(disable) interleave(disable)
          for (uint32_t i = lane; i < n; i += 64) {
            const uint8_t b = s.ring[(from + i % dist) & RMASK];
            s.ring[(pos + i) & RMASK] = b;
          }
        }
        pos += n;
      }
      if (pos - flushed >= FLUSH) flush(FLUSH);
    }
  }

  __device__ int run() {
    need32();
    const uint32_t cmf = peek(8), flg = (uint32_t)(buf >> 8) & 0xFFu;
    drop(16);
    if (exhausted()) return NBM_INFLATE_EINPUT;
    if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 32u)) return NBM_INFLATE_EHEADER;
    uint32_t last;
    do {                                                    // every block consumes at least three bits
      need32();
      last = peek(1);
      const uint32_t type = (uint32_t)(buf >> 1) & 3u;
      drop(3);
      if (exhausted()) return NBM_INFLATE_EINPUT;
      int rc;
      if (type == 0u) {
        rc = stored_block();
      } else if (type == 3u) {
        rc = NBM_INFLATE_EBLOCKTYPE;
      } else {
        rc = type == 1u ? fixed_tables() : dynamic_tables();
        if (rc == NBM_OK) rc = coded_block();
      }
      if (rc != NBM_OK) return rc;
    } while (!last);
    if (pos > flushed) flush(pos - flushed);
    drop(cnt & 7u);
    need32();
    const uint32_t t = __builtin_bswap32((uint32_t)buf);
    drop(32);
    if (exhausted()) return NBM_INFLATE_EINPUT;
    if (pos != expect) return NBM_INFLATE_EOUTPUT;
    if (t != ((adler_b << 16) | adler_a)) return NBM_INFLATE_EADLER;
    return NBM_OK;
  }
};

__global__ __launch_bounds__(64) void png_inflate_kernel(const uint8_t* __restrict__ payload, long long payload_bytes,
                                                         const long long* __restrict__ table, uint8_t* __restrict__ out,
                                                         long long out_pitch, unsigned expect, int* __restrict__ status) {
  __shared__ InflateLds s;
  const int lane = threadIdx.x;
  const long long off = table[2 * blockIdx.x], len = table[2 * blockIdx.x + 1];
  int rc;
  if (off < 0 || len < 0 || (off & 15) || len > (1ll << 30) || off > payload_bytes || len > payload_bytes - off) {
    rc = NBM_INFLATE_ETABLE;
  } else {
    Inflater inf(s, payload + off, (uint32_t)len, out + blockIdx.x * out_pitch, expect, lane);
    rc = inf.run();
  }
  if (lane == 0) status[blockIdx.x] = rc;
}

}  // namespace

extern "C" int nbm_png_inflate(const uint8_t* payload, int64_t payload_bytes, const int64_t* table, int batch,
                               uint8_t* out, int64_t out_pitch, int64_t expect, int32_t* status, void* stream) {
  if (!payload || !table || !out || !status || batch <= 0 || payload_bytes <= 0) return NBM_EINVAL;
  if (expect <= 0 || expect > (1ll << 30) || out_pitch < expect) return NBM_EINVAL;
  if (!nbm_aligned16(payload) || !nbm_aligned16(out) || (batch > 1 && (out_pitch & 15))) return NBM_EALIGN;
  hipLaunchKernelGGL(png_inflate_kernel, dim3(batch), dim3(64), 0, (hipStream_t)stream, payload, (long long)payload_bytes,
                     (const long long*)table, out, (long long)out_pitch, (unsigned)expect, status);
  return nbm_launch_status();
}
