// The host side of the mergeable latency sketch (include/isim.h isim_sketch_*,
// DESIGN.md §16): the bucket rule as functions, the merge of tables and the
// quantile brackets of one table.  No HIP: these work without a GPU.
#include <cstdint>
#include <string>

#include "../../include/isim.h"
#include "error.h"
#include "quantile_rank.h"
#include "sketch_bucket.h"

namespace {

namespace sk = isim::sk;

constexpr uint64_t kMaxCount = 1ull << 40;                              // isim_quantile_rank's limit
constexpr uint64_t kMaxRows = (uint64_t)ISIM_TL_MAX_WINDOWS + 2;

int sfail(const std::string &msg) { return isim::set_error(ISIM_EINVAL, msg); }

bool bad_sub_bits(uint32_t s) { return s > sk::kMaxSubBits; }
const char *const kSubBitsMsg = "sub_bits must be 0..7";

}  // namespace

extern "C" {

int isim_sketch_bucket(uint32_t sub_bits, uint64_t v, uint32_t *bin) {
  if (bad_sub_bits(sub_bits)) return sfail(kSubBitsMsg);
  if (!bin) return sfail("null argument");
  *bin = sk::bucket(sub_bits, v);
  return ISIM_OK;
}

int isim_sketch_bounds(uint32_t sub_bits, uint32_t bin, uint64_t *lo, uint64_t *hi) {
  if (bad_sub_bits(sub_bits)) return sfail(kSubBitsMsg);
  if (!lo || !hi) return sfail("null argument");
  if (bin >= sk::bins(sub_bits)) return sfail("bin is not below ISIM_SK_BINS(sub_bits)");
  sk::bounds(sub_bits, bin, *lo, *hi);
  return ISIM_OK;
}

int isim_sketch_merge(uint32_t sub_bits, uint64_t n_rows, uint64_t *dst, const uint64_t *src) {
  if (bad_sub_bits(sub_bits)) return sfail(kSubBitsMsg);
  if (!dst || !src) return sfail("null argument");
  if (n_rows == 0 || n_rows > kMaxRows) return sfail("n_rows must be 1.." + std::to_string(kMaxRows));
  const uint64_t words = n_rows * ISIM_SK_WORDS(sub_bits);
  for (uint64_t i = 0; i < words; ++i) dst[i] += src[i];
  return ISIM_OK;
}

int isim_sketch_quantiles(uint32_t sub_bits, const uint64_t *table, const uint32_t *q_ppm, uint32_t n_q,
                          uint64_t *out) {
  if (bad_sub_bits(sub_bits)) return sfail(kSubBitsMsg);
  if (const std::string m = isim::q::list_error(q_ppm, n_q); !m.empty()) return sfail(m);
  if (!table || !out) return sfail("null table or out");
  const uint32_t bins = sk::bins(sub_bits);
  const uint64_t *t200 = table, *t500 = table + bins;
  // the class counts; a word above 2^40 ends the sum before it can wrap
  uint64_t cnt[3] = {0, 0, 0};
  for (uint32_t b = 0; b < bins; ++b) {
    if (t200[b] > kMaxCount || t500[b] > kMaxCount) return sfail("a class count is above 2^40");
    cnt[ISIM_Q_200] += t200[b];
    cnt[ISIM_Q_500] += t500[b];
    if (cnt[ISIM_Q_200] > kMaxCount || cnt[ISIM_Q_500] > kMaxCount) return sfail("a class count is above 2^40");
  }
  cnt[ISIM_Q_ALL] = cnt[ISIM_Q_200] + cnt[ISIM_Q_500];
  if (cnt[ISIM_Q_ALL] > kMaxCount) return sfail("a class count is above 2^40");
  const uint32_t ow = (uint32_t)(ISIM_SKQ_OUT_WORDS(n_q) / 3);  // words per class: the count, then lo and hi per quantile
  for (uint32_t c = 0; c < 3; ++c) {
    uint64_t *o = out + (uint64_t)c * ow;
    for (uint32_t w = 0; w < ow; ++w) o[w] = 0;
    o[0] = cnt[c];
    if (!cnt[c]) continue;
    for (uint32_t i = 0; i < n_q; ++i) {
      const uint64_t k = isim::q::nearest_rank(cnt[c], q_ppm[i]);
      uint64_t run = 0;
      uint32_t b = 0;
      for (; b < bins; ++b) {
        run += (c != ISIM_Q_500 ? t200[b] : 0) + (c != ISIM_Q_200 ? t500[b] : 0);
        if (run >= k) break;  // k <= cnt[c], the sum over every bin: reached inside the table
      }
      sk::bounds(sub_bits, b, o[1 + 2 * i], o[2 + 2 * i]);
    }
  }
  return ISIM_OK;
}

}  // extern "C"
