// The one place the library allocates and frees device and pinned-host memory: the seam under DevBuf / HostPinned (ins_devbuf.h), with a count of what is
// live (ins_dbg_dev_live).
#include <atomic>

#include "ins_debug.h"
#include "ins_devbuf.h"
#include "ins_internal.h"

static std::atomic<int64_t> g_live_buffers{0}, g_live_bytes{0};

static int handed_out(hipError_t e, void** p, size_t bytes, const char* what) {
  if (e != hipSuccess) {
    *p = nullptr;
    (void)hipGetLastError();  // the failure is reported here: it must not surface again at the next launch check
    ins_set_error("%s of %zu bytes failed: %s", what, bytes, hipGetErrorString(e));
    return INS_ERR_HIP;
  }
  if (*p) g_live_buffers += 1, g_live_bytes += (int64_t)bytes;
  return INS_OK;
}
static void taken_back(size_t bytes) { g_live_buffers -= 1, g_live_bytes -= (int64_t)bytes; }
static int filled(hipError_t e, size_t bytes, const char* what) {
  if (e == hipSuccess) return INS_OK;
  ins_set_error("%s of %zu bytes failed: %s", what, bytes, hipGetErrorString(e));
  return INS_ERR_HIP;
}

int ins_devmem_alloc(void** p, size_t bytes) { return handed_out(hipMalloc(p, bytes), p, bytes, "hipMalloc"); }
void ins_devmem_free(void* p, size_t bytes) {
  if (!p) return;
  (void)hipFree(p);
  taken_back(bytes);
}
int ins_devmem_zero(void* p, size_t bytes) { return filled(hipMemset(p, 0, bytes), bytes, "hipMemset"); }
int ins_devmem_zero_async(void* p, size_t bytes, void* stream) { return filled(hipMemsetAsync(p, 0, bytes, as_stream(stream)), bytes, "hipMemsetAsync"); }
int ins_devmem_copy_from_host(void* dst, const void* src, size_t bytes) {
  return filled(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice), bytes, "hipMemcpy (host to device)");
}
int ins_devmem_copy_on_device(void* dst, const void* src, size_t bytes, void* stream) {
  return filled(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, as_stream(stream)), bytes, "hipMemcpyAsync (device to device)");
}
int ins_devmem_host_alloc(void** p, size_t bytes) { return handed_out(hipHostMalloc(p, bytes), p, bytes, "hipHostMalloc"); }
void ins_devmem_host_free(void* p, size_t bytes) {
  if (!p) return;
  (void)hipHostFree(p);
  taken_back(bytes);
}
void ins_devmem_live(int64_t* buffers, int64_t* bytes) {
  if (buffers) *buffers = g_live_buffers.load();
  if (bytes) *bytes = g_live_bytes.load();
}

extern "C" void ins_dbg_dev_live(int64_t* buffers, int64_t* bytes) { ins_devmem_live(buffers, bytes); }
