// Host-only check of the borrowed (non-owning) Arena of egonn_amd/csrc/common.h — the form the ICP entry points hand to the
// segmented sort over a span of the caller's scratch.  A program of its own (tests/test_entry_points_host.py builds and runs
// it): it links nothing of the library, so the error sink is defined here.
#include <stdarg.h>
#include <stdlib.h>

#include "../egonn_amd/csrc/common.h"

static char g_msg[512];
namespace egonn {
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
  va_end(ap);
}
}  // namespace egonn

#define CHECK(cond)                                            \
  do {                                                         \
    if (!(cond)) {                                             \
      printf("FAILED line %d: %s\n", __LINE__, #cond);         \
      return 1;                                                \
    }                                                          \
  } while (0)

int main() {
  const size_t cap = 4096;
  char* span = static_cast<char*>(malloc(cap));
  CHECK(span);
  memset(span, 0x5A, cap);
  egonn::Arena a = egonn::Arena::view(span, cap);
  CHECK(a.borrowed && a.base == span && a.cap == cap && a.off == 0);
  CHECK(a.ensure(cap) == EGONN_OK);
  CHECK(a.base == span && a.cap == cap);
  // carves: aligned to 256 inside the span, null beyond it
  int32_t* p0 = a.alloc<int32_t>(10);
  int32_t* p1 = a.alloc<int32_t>(10);
  CHECK((char*)p0 == span && (char*)p1 == span + 256);
  CHECK(a.alloc<char>(cap) == nullptr);
  // one byte too many: an error that names the shortfall; nothing synchronised, freed, allocated or moved
  g_msg[0] = 0;
  CHECK(a.ensure(cap + 1) == EGONN_ERR_INVALID);
  CHECK(strstr(g_msg, "1 bytes short") && strstr(g_msg, "4096") && strstr(g_msg, "4097"));
  CHECK(a.base == span && a.cap == cap && a.borrowed);
  a.release();
  CHECK(a.base == span && a.cap == cap);
  for (size_t i = 0; i < cap; ++i) CHECK(span[i] == 0x5A);   // still the caller's memory, untouched
  free(span);                                                 // and still the caller's to free
  printf("borrowed arena: ok\n");
  return 0;
}
