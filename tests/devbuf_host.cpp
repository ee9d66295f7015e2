// Stand-alone check of DevBuf / HostPinned (csrc/ins_devbuf.h) on the host: this file defines the seam over malloc / free, with a live counter and a
// "fail the N-th allocation" switch, and is built with -fsanitize=address,undefined by tests/test_devbuf_host.py.  Exit status 0: every check held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "ins_devbuf.h"

static int64_t g_buffers = 0, g_bytes = 0;
static int g_allocs = 0, g_fail_at = 0;  // g_fail_at = N > 0: the N-th allocation from now fails

static int seam_alloc(void** p, size_t bytes) {
  *p = nullptr;
  if (g_fail_at > 0 && ++g_allocs == g_fail_at) return INS_ERR_HIP;
  if (bytes == 0) return INS_OK;
  *p = malloc(bytes);
  if (!*p) return INS_ERR_HIP;
  memset(*p, 0xa5, bytes);  // fresh memory is not zero: the zero forms have to do it
  g_buffers += 1, g_bytes += (int64_t)bytes;
  return INS_OK;
}
static void seam_free(void* p, size_t bytes) {
  if (!p) return;
  free(p);
  g_buffers -= 1, g_bytes -= (int64_t)bytes;
}
int ins_devmem_alloc(void** p, size_t bytes) { return seam_alloc(p, bytes); }
void ins_devmem_free(void* p, size_t bytes) { seam_free(p, bytes); }
int ins_devmem_zero(void* p, size_t bytes) { return memset(p, 0, bytes), INS_OK; }
int ins_devmem_zero_async(void* p, size_t bytes, void*) { return memset(p, 0, bytes), INS_OK; }
int ins_devmem_copy_from_host(void* dst, const void* src, size_t bytes) { return memcpy(dst, src, bytes), INS_OK; }
int ins_devmem_copy_on_device(void* dst, const void* src, size_t bytes, void*) { return memcpy(dst, src, bytes), INS_OK; }
int ins_devmem_host_alloc(void** p, size_t bytes) { return seam_alloc(p, bytes); }
void ins_devmem_host_free(void* p, size_t bytes) { seam_free(p, bytes); }
void ins_devmem_live(int64_t* buffers, int64_t* bytes) { *buffers = g_buffers, *bytes = g_bytes; }

static int g_failed = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                    \
    }                                                                \
  } while (0)

static bool live(int64_t buffers, int64_t bytes) {
  int64_t n, b;
  ins_devmem_live(&n, &b);
  return n == buffers && b == bytes;
}

// a handle with several buffers, filled the way the create functions do it: the first failure stops the chain
struct Handle {
  DevBuf<double> a;
  DevBuf<float> b[2];
  std::vector<DevBuf<double>> k;
  HostPinned<double> h;
  DevBuf<int> c;
  static constexpr int members = 8;
  int create() {
    int rc;
    k.resize(3);
    if ((rc = a.alloc_zero(7)) || (rc = b[0].alloc(5)) || (rc = b[1].alloc_zero_async(5, nullptr))) return rc;
    for (auto& ki : k)
      if ((rc = ki.alloc_zero(11))) return rc;
    if ((rc = h.alloc(4))) return rc;
    const int src[3] = {1, 2, 3};
    return c.alloc_copy_host(3, src);
  }
};

int main() {
  {  // the null state, and what an allocation holds
    DevBuf<double> d;
    CHECK(d.get() == nullptr && d.count() == 0 && !d && live(0, 0));
    CHECK(d.alloc(10) == INS_OK && d.get() && d.count() == 10 && live(1, 80));
    double* raw = d;  // the implicit conversion
    CHECK(raw == d.get());
    d.reset();
    CHECK(!d && d.count() == 0 && live(0, 0));
    d.reset();  // twice is harmless
    CHECK(live(0, 0));
  }
  {  // the filled forms
    DevBuf<double> z;
    CHECK(z.alloc_zero(6) == INS_OK);
    for (int i = 0; i < 6; ++i) CHECK(z[i] == 0.0);
    CHECK(z.alloc_zero_async(9, nullptr) == INS_OK && z.count() == 9 && live(1, 72));  // a second allocation frees the first
    for (int i = 0; i < 9; ++i) CHECK(z[i] == 0.0);
    const double src[4] = {1.5, -2.0, 3.25, 4.0};
    DevBuf<double> c, e;
    CHECK(c.alloc_copy_host(4, src) == INS_OK && e.alloc_copy_device(4, c, nullptr) == INS_OK);
    for (int i = 0; i < 4; ++i) CHECK(c[i] == src[i] && e[i] == src[i]);
    CHECK(live(3, 72 + 32 + 32));
    DevBuf<double> none;
    CHECK(none.alloc_zero(0) == INS_OK && !none && none.count() == 0);  // nothing to hold
  }
  CHECK(live(0, 0));
  {  // moves
    DevBuf<int> a;
    CHECK(a.alloc(3) == INS_OK);
    int* pa = a;
    DevBuf<int> b(std::move(a));
    CHECK(!a && a.count() == 0 && b.get() == pa && b.count() == 3 && live(1, 12));
    DevBuf<int> c;
    CHECK(c.alloc(8) == INS_OK && live(2, 44));
    c = std::move(b);  // frees what c held
    CHECK(!b && c.get() == pa && c.count() == 3 && live(1, 12));
    DevBuf<int>& self = c;
    c = std::move(self);  // self-move keeps the buffer
    CHECK(c.get() == pa && c.count() == 3 && live(1, 12));
    std::vector<DevBuf<int>> v(2);
    CHECK(v[1].alloc(2) == INS_OK);
    int* pv = v[1];
    v.resize(64);  // reallocation moves the owners, not the buffers
    CHECK(v[1].get() == pv && live(2, 20));
    HostPinned<double> h, g;
    CHECK(h.alloc(4) == INS_OK && live(3, 52));
    double* ph = h;
    g = std::move(h);
    CHECK(!h && g.get() == ph && g.count() == 4);
    HostPinned<double>& gs = g;
    g = std::move(gs);
    CHECK(g.get() == ph && live(3, 52));
  }
  CHECK(live(0, 0));
  {  // ensure: larger reallocates, equal and smaller keep the address
    DevBuf<double> s;
    CHECK(s.ensure(16) == INS_OK && s.count() == 16 && live(1, 128));
    double* p0 = s;
    CHECK(s.ensure(16) == INS_OK && s.get() == p0 && s.count() == 16);
    CHECK(s.ensure(4) == INS_OK && s.get() == p0 && s.count() == 16 && live(1, 128));
    CHECK(s.ensure(17) == INS_OK && s.count() == 17 && live(1, 136));
  }
  CHECK(live(0, 0));
  {  // a failed allocation leaves the buffer null, whatever it held
    DevBuf<double> d;
    CHECK(d.alloc(4) == INS_OK);
    g_allocs = 0, g_fail_at = 1;
    CHECK(d.alloc_zero(8) == INS_ERR_HIP && !d && d.count() == 0 && live(0, 0));
    g_allocs = 0, g_fail_at = 1;
    CHECK(d.ensure(8) == INS_ERR_HIP && !d);
    g_allocs = 0, g_fail_at = 1;
    HostPinned<double> h;
    CHECK(h.alloc(8) == INS_ERR_HIP && !h && live(0, 0));
    g_fail_at = 0;
  }
  // a handle whose N-th allocation fails holds nothing once it is destroyed, for every N; and without a failure it holds all its members
  for (int n = 0; n <= Handle::members; ++n) {
    g_allocs = 0, g_fail_at = n;
    {
      Handle H;
      const int rc = H.create();
      CHECK((rc == INS_OK) == (n == 0));
      if (n == 0) CHECK(live(Handle::members, 7 * 8 + 2 * 5 * 4 + 3 * 11 * 8 + 4 * 8 + 3 * 4) && H.c[2] == 3);
      if (n > 0) CHECK(g_allocs == n);  // the chain stopped at the failure
    }
    CHECK(live(0, 0));
  }
  g_fail_at = 0;
  if (g_failed) fprintf(stderr, "%d checks failed\n", g_failed);
  return g_failed ? 1 : 0;
}
