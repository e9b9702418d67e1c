// The batched fp64 linear algebra (oi_linalg.h) through a C entry layer, for
// the tests only (tests/oila_ref.py binds it with ctypes): each call stages the
// caller's descriptors -- DEVICE pointers -- runs one oila:: routine on the
// caller's stream and returns once the stream has drained.  The names are not
// part of include/oi.h.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "oi_host.h"
#include "oi_linalg.h"

namespace {

// oi_guarded's mapping with the routine's name in front of the text; the
// stream is drained before the descriptor ring is destroyed
template <class F>
int guarded(void* stream, const char* what, F&& run) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  oila::Stager S;
  S.bind(st);
  int rc = oi_guarded([&] {
    run(S, st);
    return 0;
  });
  if (rc) rc = oi_set_last_error(rc, (std::string(what) + ": " + oi_last_error()).c_str());
  const hipError_t err = hipStreamSynchronize(st);
  if (rc == 0 && err != hipSuccess)
    rc = oi_set_last_error(OI_E_HIP, (std::string(what) + ": " + hipGetErrorString(err)).c_str());
  return rc;
}

template <class T>
std::vector<T> vec(const T* p, int count) {
  return std::vector<T>(p, p + count);
}

}  // namespace

extern "C" {

// which: 0 Gemm, 1 Gemv, 2 Chol, 3 TrsmRLT, 4 Eigh (the ctypes mirrors are checked against these)
int oila_test_sizeof(int which) {
  switch (which) {
    case 0: return (int)sizeof(oila::Gemm);
    case 1: return (int)sizeof(oila::Gemv);
    case 2: return (int)sizeof(oila::Chol);
    case 3: return (int)sizeof(oila::TrsmRLT);
    case 4: return (int)sizeof(oila::Eigh);
  }
  return -1;
}

int oila_test_gemm(const oila::Gemm* g, int count, int ta, int tb, void* stream) {
  if (count < 0 || (count > 0 && !g)) return oi_set_last_error(OI_E_ARG, "oila_test_gemm: bad arguments");
  return guarded(stream, "oila_test_gemm",
                 [&](oila::Stager& S, hipStream_t st) { oila::gemm(S, st, ta != 0, tb != 0, vec(g, count)); });
}

int oila_test_gemv(const oila::Gemv* g, int count, int trans, void* stream) {
  if (count < 0 || (count > 0 && !g)) return oi_set_last_error(OI_E_ARG, "oila_test_gemv: bad arguments");
  return guarded(stream, "oila_test_gemv",
                 [&](oila::Stager& S, hipStream_t st) { oila::gemv(S, st, trans != 0, vec(g, count)); });
}

int oila_test_cholesky(const oila::Chol* c, int count, void* stream) {
  if (count < 0 || (count > 0 && !c)) return oi_set_last_error(OI_E_ARG, "oila_test_cholesky: bad arguments");
  return guarded(stream, "oila_test_cholesky",
                 [&](oila::Stager& S, hipStream_t st) { oila::cholesky(S, st, vec(c, count)); });
}

int oila_test_trsm_right_lt(const oila::TrsmRLT* t, int count, void* stream) {
  if (count < 0 || (count > 0 && !t)) return oi_set_last_error(OI_E_ARG, "oila_test_trsm_right_lt: bad arguments");
  return guarded(stream, "oila_test_trsm_right_lt",
                 [&](oila::Stager& S, hipStream_t st) { oila::trsm_right_lt(S, st, vec(t, count)); });
}

int oila_test_eigh(const oila::Eigh* e, int count, void* stream) {
  if (count < 0 || (count > 0 && !e)) return oi_set_last_error(OI_E_ARG, "oila_test_eigh: bad arguments");
  return guarded(stream, "oila_test_eigh",
                 [&](oila::Stager& S, hipStream_t st) { oila::eigh(S, st, vec(e, count)); });
}

long long oila_test_eigh_workspace_doubles(int M) {
  return M < 0 ? -1 : (long long)oila::eigh_workspace_doubles(M);
}

}  // extern "C"
