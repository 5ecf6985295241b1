// C-ABI (include/fts_gpu.h): the stand-alone G1 MSM (BASELINE config C3).
#include "host/api_internal.hpp"

struct fts_msm_batch {
  int N = 0;
  int device = 0;
  DevBuf pts_mem, sc_mem, out_mem;
  uint32_t* pts = nullptr;  // [N][16] affine Montgomery
  uint32_t* sc = nullptr;   // [N][8] canonical scalars
  uint8_t* out = nullptr;   // 64-byte result
  bool alloc(size_t n) {
    if (!pts_mem.reserve(n * 64) || !sc_mem.reserve(n * 32) || !out_mem.reserve(64)) return false;
    pts = pts_mem.as<uint32_t>(), sc = sc_mem.as<uint32_t>(), out = out_mem.as<uint8_t>();
    return true;
  }
  ~fts_msm_batch() { hipSetDevice(device); }
  TimingRecord tim;
};
extern "C" {

void fts_msm_free(fts_msm_batch* b) { delete b; }

int fts_msm_stage(fts_ctx* c, size_t n, const uint8_t* points64, const uint8_t* scalars32, fts_msm_batch** out) {
  if (c && !c->shards.empty()) return fts_msm_stage(c->shards[0], n, points64, scalars32, out);
  if (!c || !out || !n || !points64 || !scalars32 || n > (size_t)(1u << 26)) return FTS_API_EINVAL;
  if (c->device < 0) return FTS_API_EDEVICE;
  HIP_OK(hipSetDevice(c->device));
  std::unique_ptr<fts_msm_batch> b(new fts_msm_batch());
  b->N = (int)n;
  b->device = c->device;
  DevBuf rp, rs, bad;  // the raw inputs, released (with the null stream drained) on every exit
  if (!b->alloc(n) || !rp.reserve(n * 64) || !rs.reserve(n * 32) || !bad.reserve(4)) return FTS_API_ENOMEM;
  uint32_t nbad = 0;
  hipError_t e = hipMemcpy(rp.p, points64, n * 64, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(rs.p, scalars32, n * 32, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(bad.p, 0, 4);
  if (e == hipSuccess) {
    launch_msm_load((int)n, rp.as<uint8_t>(), rs.as<uint8_t>(), b->pts, b->sc, bad.as<uint32_t>(), 0);
    e = hipMemcpy(&nbad, bad.p, 4, hipMemcpyDeviceToHost);
  }
  if (e != hipSuccess) return FTS_API_EDEVICE;
  if (nbad) return FTS_API_EINVAL;  // a point failed NewG1FromBytes (flags, range, on-curve)
  *out = b.release();
  return FTS_API_OK;
}

int fts_msm_stage_multiples(fts_ctx* c, size_t n, const uint8_t* k32, const uint8_t* scalars32, fts_msm_batch** out) {
  if (c && !c->shards.empty()) return fts_msm_stage_multiples(c->shards[0], n, k32, scalars32, out);
  if (!c || !out || !n || !k32 || !scalars32 || n > (size_t)(1u << 26)) return FTS_API_EINVAL;
  if (c->device < 0) return FTS_API_EDEVICE;
  HIP_OK(hipSetDevice(c->device));
  std::unique_ptr<fts_msm_batch> b(new fts_msm_batch());
  b->N = (int)n;
  b->device = c->device;
  if (!b->alloc(n)) return FTS_API_ENOMEM;
  // the temporaries on a private stream with stream-ordered allocation, synchronised
  // alone: a device-wide sync (hipDeviceSynchronize, or hipFree) here would stall
  // every lane's in-flight pass on a shared context
  uint8_t *rk = nullptr, *rs = nullptr;
  uint32_t* jac = nullptr;
  hipStream_t st = nullptr;
  hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipMallocAsync((void**)&rk, n * 32, st);
  if (e == hipSuccess) e = hipMallocAsync((void**)&rs, n * 32, st);
  if (e == hipSuccess) e = hipMallocAsync((void**)&jac, n * 96, st);
  if (e == hipSuccess) e = hipMemcpyAsync(rk, k32, n * 32, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(rs, scalars32, n * 32, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    // B = the PP's ped[1] (table slot tb_G): a generator of G1
    launch_msm_gen_points((int)n, rk, rs, c->d_tables.as<uint32_t>() + (size_t)tb_G(c->n) * fb_words_per_base(), jac, b->pts, b->sc,
                          st);
    e = hipGetLastError();
  }
  for (void* p : {(void*)rk, (void*)rs, (void*)jac})
    if (p) (void)hipFreeAsync(p, st);
  if (st) {
    const hipError_t e2 = hipStreamSynchronize(st);
    if (e == hipSuccess) e = e2;
    hipStreamDestroy(st);
  }
  if (e != hipSuccess) return e == hipErrorOutOfMemory ? FTS_API_ENOMEM : FTS_API_EDEVICE;
  *out = b.release();
  return FTS_API_OK;
}

int fts_msm_points(fts_ctx* c, const fts_msm_batch* b, size_t lo, size_t count, uint8_t* out64) {
  if (c && !c->shards.empty()) return fts_msm_points(c->shards[0], b, lo, count, out64);
  if (!c || !b || (count && !out64) || lo > (size_t)b->N || count > (size_t)b->N - lo) return FTS_API_EINVAL;
  if (c->device < 0) return FTS_API_EDEVICE;
  if (!count) return FTS_API_OK;
  HIP_OK(hipSetDevice(c->device));
  // private stream and stream-ordered scratch: no device-wide sync (see fts_msm_stage_multiples)
  hipStream_t st = nullptr;
  uint8_t* d = nullptr;
  hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipMallocAsync((void**)&d, count * 64, st);
  if (e == hipSuccess) {
    launch_msm_pts_to_bytes((int)count, b->pts + lo * 16, d, st);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out64, d, count * 64, hipMemcpyDeviceToHost, st);
  if (d) (void)hipFreeAsync(d, st);
  if (st) {
    const hipError_t e2 = hipStreamSynchronize(st);
    if (e == hipSuccess) e = e2;
    hipStreamDestroy(st);
  }
  return e == hipSuccess ? FTS_API_OK : FTS_API_EDEVICE;
}

int fts_msm_run(fts_ctx* c, fts_msm_batch* b, uint8_t* out64) {
  if (c && !c->shards.empty()) return fts_msm_run(c->shards[0], b, out64);
  if (!c || !b || !out64) return FTS_API_EINVAL;
  if (c->device < 0) return FTS_API_EDEVICE;
  HIP_OK(hipSetDevice(c->device));
  LaneGuard lg(c);
  Lane& L = *lg.L;
  MsmPlan mp{};
  // standalone MSMs: the block-local counting sort; from 2^20 points 32-point
  // chunks (~8 partials per bucket instead of ~32 at 2^22)
  if (int rc = msm_prepare(L, b->N, mp, MSM_SLOT_PASS, b->N >= (1 << 20) ? 32 : MSM_CH, c->msm_sort != 0, c->msm_maxc))
    return rc;
  L.tl.begin(L.s);
  launch_msm(mp, b->pts, b->sc, nullptr, 0, L.ws.m_scratch.as<uint32_t>(), L.s, L.s, &L.tl);
  launch_msm_to_bytes(mp.out, b->out, L.s);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(out64, b->out, 64, hipMemcpyDeviceToHost, L.s));
  HIP_OK(L.sync());
  b->tim.n = 0;
  b->tim.add_marks(L.tl);
  return FTS_API_OK;
}

int fts_msm_timings(const fts_msm_batch* b, const char** names, float* ms, double* mads, int cap) {
  if (!b) return 0;
  return b->tim.copy_out(names, ms, mads, cap);
}

int fts_msm_g1(fts_ctx* c, size_t n, const uint8_t* points64, const uint8_t* scalars32, uint8_t* out64) {
  if (!out64) return FTS_API_EINVAL;
  if (n == 0) {
    memset(out64, 0, 64);
    return FTS_API_OK;
  }
  if (c && !c->shards.empty()) {
    // partial MSM per device, the partial points combined on the host
    const std::vector<size_t> bnd = plan(n, nullptr, (int)c->shards.size());
    std::vector<uint8_t> part(64 * c->shards.size(), 0);
    int rc = run_shards(bnd, [&](int j, size_t lo, size_t hi) {
      return fts_msm_g1(c->shards[j], hi - lo, points64 + 64 * lo, scalars32 + 32 * lo, &part[64 * j]);
    });
    if (rc != FTS_API_OK) return rc;
    G1J acc = jac_identity();
    for (size_t j = 0; j < c->shards.size(); j++) {
      G1A a;
      if (!g1_from_bytes(&part[64 * j], 64, a)) return FTS_API_EDEVICE;
      acc = jadd_aff(acc, a);
    }
    g1_to_bytes(to_aff(acc), out64);
    return FTS_API_OK;
  }
  fts_msm_batch* b = nullptr;
  int rc = fts_msm_stage(c, n, points64, scalars32, &b);
  if (rc != FTS_API_OK) return rc;
  rc = fts_msm_run(c, b, out64);
  fts_msm_free(b);
  return rc;
}

}  // extern "C"
