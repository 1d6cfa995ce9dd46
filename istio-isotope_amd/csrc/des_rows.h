// The DES level engine's rows on the device: the row type,
// the one load and the one store of a thread's kPer consecutive values, and
// the change tracking of the fixed-point passes.
//
// Included by des.hip INSIDE namespace isim::dev, after DesK (as des_draw.h:
// a piece of that translation unit, not a header of its own).

// ---- rows: u32 (narrow) or u64, times relative to A_t, status in the top bit
template <typename T>
struct Row {
  static constexpr uint32_t kTop = 8 * sizeof(T) - 1;
  static constexpr uint64_t kSt = 1ull << kTop;
  static constexpr uint64_t kMask = kSt - 1;
  // narrow rows hold values below 2^31 (the status bit stays free)
  __device__ static bool fits(uint64_t v) { return sizeof(T) == 8 || v < kSt; }
};

template <typename T>
__device__ __forceinline__ T *row(void *base, uint64_t ld, uint32_t r) {
  return reinterpret_cast<T *>(base) + (uint64_t)r * ld;
}

// ---- row access: the values [base, base + kPer) of a row (base % kPer == 0,
// so 16-B aligned), in the row type — a caller that needs 64-bit values widens
// them itself.  The call says which of the values lie below n and how the
// access goes through the caches; each instruction choice is made here once.
enum class Quad {
  whole,  // all of them, the caller knows: one 16-B access per 16 B, n is not read
  test,   // tested here: as `whole` when base + kPer <= n, else as `each`
  each,   // value by value, those below n (a load gives 0 past n)
};
enum class Mem {
  plain,
  // stores of narrow rows: the 16-B store is nontemporal, which keeps L2 for
  // the A_t re-reads (the rows are read next by a later launch); the
  // value-by-value tail is plain
  nontemporal,
  // Rows handed between workgroups inside a launch (des_down_pipe), the sc1
  // form of the guide's Guideline 16: the producer's 16-B stores are sc1
  // (write-through), drained by every storing wave before the barrier behind
  // which one lane stores the flag (sc1); the consumer polls the flag with sc1
  // loads and reads every handed-off byte with sc1 loads (L1 bypassed), so no
  // release or acquire fence.  A buffer resource per chunk of kPer x
  // kDownThreads values from c0 keeps the offsets 32-bit; value by value the
  // accesses are agent-scope relaxed atomics.
  sc1,
};
// the store of a row by the pass that computes it: narrow rows nontemporal;
// wide rows have only been measured with plain stores
template <typename T>
constexpr Mem kRowStore = sizeof(T) == 4 ? Mem::nontemporal : Mem::plain;

typedef uint32_t des_v4u __attribute__((ext_vector_type(4)));
constexpr int kRsrcWord3 = 0x00020000;  // gfx9 raw buffer: 32-bit data format, no swizzle
constexpr int kSc1 = 16;                // cache-policy aux bit of the buffer builtins

template <typename T, Quad Q, Mem M = Mem::plain>
__device__ __forceinline__ void load_row(const T *p, uint64_t base, uint64_t n, T (&x)[kPer], uint64_t c0 = 0) {
  static_assert(M != Mem::nontemporal, "rows are not loaded nontemporally");
  if (Q == Quad::whole || (Q == Quad::test && base + kPer <= n)) {
    if constexpr (M == Mem::sc1) {
      const __amdgpu_buffer_rsrc_t r =
          __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(p + c0), (short)0, (int)(sizeof(T) * kPer * kDownThreads),
                                            kRsrcWord3);
      const uint32_t vo = (uint32_t)(base - c0) * (uint32_t)sizeof(T);
      if constexpr (sizeof(T) == 4) {
        const des_v4u w = __builtin_amdgcn_raw_buffer_load_b128(r, vo, 0, kSc1);
        x[0] = w.x;
        x[1] = w.y;
        x[2] = w.z;
        x[3] = w.w;
      } else {
        const des_v4u w0 = __builtin_amdgcn_raw_buffer_load_b128(r, vo, 0, kSc1);
        const des_v4u w1 = __builtin_amdgcn_raw_buffer_load_b128(r, vo + 16, 0, kSc1);
        x[0] = (T)w0.x | ((T)w0.y << (4 * sizeof(T)));
        x[1] = (T)w0.z | ((T)w0.w << (4 * sizeof(T)));
        x[2] = (T)w1.x | ((T)w1.y << (4 * sizeof(T)));
        x[3] = (T)w1.z | ((T)w1.w << (4 * sizeof(T)));
      }
    } else if constexpr (sizeof(T) == 4) {
      const uint4 v = *reinterpret_cast<const uint4 *>(p + base);
      x[0] = v.x;
      x[1] = v.y;
      x[2] = v.z;
      x[3] = v.w;
    } else {
      const ulonglong2 a = reinterpret_cast<const ulonglong2 *>(p + base)[0];
      const ulonglong2 b = reinterpret_cast<const ulonglong2 *>(p + base)[1];
      x[0] = a.x;
      x[1] = a.y;
      x[2] = b.x;
      x[3] = b.y;
    }
  } else {
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i) {
      if constexpr (M == Mem::sc1)
        x[i] = base + i < n ? __hip_atomic_load(p + base + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : (T)0;
      else
        x[i] = base + i < n ? p[base + i] : (T)0;
    }
  }
}

template <typename T, Quad Q, Mem M = Mem::plain>
__device__ __forceinline__ void store_row(T *p, uint64_t base, uint64_t n, const T (&x)[kPer], uint64_t c0 = 0) {
  static_assert(M != Mem::nontemporal || sizeof(T) == 4, "nontemporal stores: narrow rows only");
  if (Q == Quad::whole || (Q == Quad::test && base + kPer <= n)) {
    if constexpr (M == Mem::sc1) {
      const __amdgpu_buffer_rsrc_t r =
          __builtin_amdgcn_make_buffer_rsrc(p + c0, (short)0, (int)(sizeof(T) * kPer * kDownThreads), kRsrcWord3);
      const uint32_t vo = (uint32_t)(base - c0) * (uint32_t)sizeof(T);
      if constexpr (sizeof(T) == 4) {
        const des_v4u w = {x[0], x[1], x[2], x[3]};
        __builtin_amdgcn_raw_buffer_store_b128(w, r, vo, 0, kSc1);
      } else {
        const des_v4u w0 = {(uint32_t)x[0], (uint32_t)((uint64_t)x[0] >> 32), (uint32_t)x[1],
                            (uint32_t)((uint64_t)x[1] >> 32)};
        const des_v4u w1 = {(uint32_t)x[2], (uint32_t)((uint64_t)x[2] >> 32), (uint32_t)x[3],
                            (uint32_t)((uint64_t)x[3] >> 32)};
        __builtin_amdgcn_raw_buffer_store_b128(w0, r, vo, 0, kSc1);
        __builtin_amdgcn_raw_buffer_store_b128(w1, r, vo + 16, 0, kSc1);
      }
    } else if constexpr (M == Mem::nontemporal) {
      __builtin_nontemporal_store(des_v4u{x[0], x[1], x[2], x[3]}, reinterpret_cast<des_v4u *>(p + base));
    } else if constexpr (sizeof(T) == 4) {
      *reinterpret_cast<uint4 *>(p + base) = make_uint4(x[0], x[1], x[2], x[3]);
    } else {
      reinterpret_cast<ulonglong2 *>(p + base)[0] = make_ulonglong2(x[0], x[1]);
      reinterpret_cast<ulonglong2 *>(p + base)[1] = make_ulonglong2(x[2], x[3]);
    }
  } else {
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i)
      if (base + i < n) {
        if constexpr (M == Mem::sc1) __hip_atomic_store(p + base + i, x[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else p[base + i] = x[i];
      }
  }
}

// stores of row values; in fixed-point passes a changed value is flagged
template <typename T, Quad Q = Quad::test>
__device__ __forceinline__ void track4(const DesK &k, const T *p, uint64_t base, uint64_t n, const T (&x)[kPer]) {
  if (!k.changed) return;
  T o[kPer];
  load_row<T, Q>(p, base, n, o);
  bool d = false;
#pragma unroll
  for (uint32_t i = 0; i < kPer; ++i) d |= (Q == Quad::whole || base + i < n) && o[i] != x[i];
  if (d) atomicOr(k.changed, 1u);
}
template <typename T>
__device__ __forceinline__ void track1(const DesK &k, const T *p, T x) {
  if (k.changed && *p != x) atomicOr(k.changed, 1u);
}

__device__ __forceinline__ void flag_overflow(const DesK &k, bool bad) {
  if (bad) atomicOr(k.ovf, 1u);
}

// the time every row value of trace t is relative to: its group's first arrival
constexpr uint64_t kDesGrp = kDesGroupTraces;  // a trace group = one DPP row of the 32-bit-key queue pass
__device__ __forceinline__ uint64_t des_gbase(const DesK &k, uint64_t t) { return k.A[t & ~(kDesGrp - 1)]; }

// relative arrival of position v (pp = pos[v]) for trace t
template <typename T>
__device__ __forceinline__ uint64_t des_arrival(const DesK &k, uint32_t v, const DesPos &pp, uint64_t t) {
  if (pp.parent == kDesNoParent) return k.A[t] - des_gbase(k, t);
  const uint32_t b = k.ext[v].bk_in;
  const T *r = b == kDesNone ? row<T>(k.W, k.ld, pp.parent) : row<T>(k.BK, k.ld, b);
  return (uint64_t)r[t] + pp.off;
}

// the row a position's arrivals are read from (null: the entry, arrival 0)
template <typename T>
__device__ __forceinline__ const T *arrival_row(const DesK &k, uint32_t v, const DesPos &pp) {
  if (pp.parent == kDesNoParent) return nullptr;
  const uint32_t b = k.ext[v].bk_in;
  return b == kDesNone ? row<T>(k.W, k.ld, pp.parent) : row<T>(k.BK, k.ld, b);
}
