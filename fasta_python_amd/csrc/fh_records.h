// fh_records.h -- the tail of a launch, written ONCE for every operator form of the second tier: block sum -> one record per workgroup -> the last
// workgroup to arrive adds the records in index order -> scalar block, sequence number, counter reset (finish_records), and its pieces for the
// launches that only hand records on (publish_record) or add those of an earlier launch (add_records, add_column).  Device code, on top of
// fh_device.h's block_reduce, store_partial / load_partial, arrive_last, scal_store and publish_seq; the element arithmetic that fills the
// records is fh_nside.h.  Kernels that keep a finaliser of their own: k_fwd_dense and k_diff_sq (held to byte-identical code), k_spmc_fwd (an
// occupancy step), k_qd_fwd and k_id_adj (a quarter of a microsecond per small launch) -- each says so where it stands, figures in profiles/nside_refactor.txt -- and the
// four whose records are not of this shape: k_gterms, k_mc_gterms and k_nuc_sigma (two or three doubles, packed), k_sm_finish (no own record).
#pragma once
#include "fh_device.h"

// ---- records ------------------------------------------------------------------------------------------------------------------------------
// A record is what one workgroup hands to the launch's finaliser: K doubles, 8 doubles apart (one double: packed).  Slot MAXSLOT (or -1) of a
// record is a maximum, every other slot a sum.  Every hand-off goes through store_partial / load_partial (fh_device.h: write-through, agent scope).

// block sum of v, then thread 0 writes record `rec` of `red`
template <int K, int MAXSLOT>
__device__ __forceinline__ void publish_record(double (&v)[K], double* red, uint32_t rec, double* scr) {
  block_reduce<K>(v, scr, MAXSLOT < K ? MAXSLOT : -1);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) store_partial(red + (uint64_t)rec * (K == 1 ? 1 : 8) + k, v[k]);
  }
}

// slots [K0, K1) of the 8-double records 0 .. n-1 into w[K0 .. K1), in index order: lane t adds records t, t + 256, ...
template <int K0, int K1, int MAXSLOT, int KW>
__device__ __forceinline__ void add_records(double (&w)[KW], const double* red, uint32_t n) {
  static_assert(0 <= K0 && K0 < K1 && K1 <= KW, "slots inside w");
  for (uint32_t i = threadIdx.x; i < n; i += FH_WG) {
#pragma unroll
    for (int k = K0; k < K1; ++k) {
      const double t = load_partial(red + (uint64_t)i * 8 + k);
      if (k == MAXSLOT) w[k] = fmax(w[k], t); else w[k] += t;
    }
  }
}
// n one-double records (a loss sum per workgroup of an earlier launch, or of this one) into one slot
__device__ __forceinline__ void add_column(double& w, const double* red, uint32_t n) {
  for (uint32_t i = threadIdx.x; i < n; i += FH_WG) w += load_partial(red + i);
}

struct NoRecords { template <int KW> __device__ __forceinline__ void operator()(double (&)[KW]) const {} };

// The finaliser of a launch.  Every workgroup: block sum of v, record `rec` of `red` (nrec records, one per arrival at `counter`).  The last
// workgroup to arrive: w[KW] = the records' slots 0 .. K-1 in index order, more(w) adds what other record arrays hold (NoRecords: nothing),
// block sum, then thread 0 alone: store(w) writes the scalar block, the sequence number follows it, the counter is zero again for the next launch.
// seq = 0: no sequence number is published and `out` is not touched here -- a launch whose result is not the scalar block passes out = nullptr.
template <int K, int MAXSLOT, int KW = K, class More, class Store>
__device__ __forceinline__ void finish_records(double (&v)[K], double* red, uint32_t rec, uint32_t nrec, unsigned* counter, double* out, unsigned seq,
                                               double* scr, unsigned* flag, More more, Store store) {
  static_assert(KW >= K, "the final sum holds every slot of a record");
  publish_record<K, MAXSLOT>(v, red, rec, scr);
  if (!arrive_last(counter, nrec, flag)) return;
  double w[KW];
#pragma unroll
  for (int k = 0; k < KW; ++k) w[k] = 0.0;
  if constexpr (K == 1) add_column(w[0], red, nrec);
  else add_records<0, K, MAXSLOT>(w, red, nrec);
  more(w);
  block_reduce<KW>(w, scr, MAXSLOT);
  if (threadIdx.x == 0) {
    store(w);
    if (seq) publish_seq(out, seq);
    __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// the usual last steps: the forward half of the scalar block (w in its order) and FH_S_ALPHA; the adjoint half (w = dxdg, dg2, xh2, gsum, gmax, fsq)
__device__ __forceinline__ void store_fwd_scalars(double* out, const double (&w)[8], double alpha) {
#pragma unroll
  for (int k = 0; k < 8; ++k) scal_store(out + k, w[k]);
  scal_store(out + S_ALPHA, alpha);
}
__device__ __forceinline__ void store_adj_scalars(double* out, const double (&w)[6]) {
  scal_store(out + S_DXDG, w[0]); scal_store(out + S_DG2, w[1]); scal_store(out + S_XH2_ADJ, w[2]);
  scal_store(out + S_GSUM_ADJ, w[3]); scal_store(out + S_GMAX_ADJ, w[4]); scal_store(out + S_FSQ_ADJ, w[5]);
}
