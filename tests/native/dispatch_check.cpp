// Self-test of the host-side dispatch helpers (pnode_amd/csrc/pn_dispatch.h), meant to run under
// -fsanitize=address,undefined: a count mapped to the wrong instantiation hands a kernel the null tail of its
// argument struct, which on a device is a fault and here is a failed comparison.
#include <cstdio>
#include <type_traits>

#include "pn_dispatch.h"

static int g_fail = 0;
#define CHECK(...)                                                    \
  do {                                                                \
    if (!(__VA_ARGS__)) {                                             \
      std::printf("FAILED line %d: %s\n", __LINE__, #__VA_ARGS__);    \
      ++g_fail;                                                       \
    }                                                                 \
  } while (0)

// with_count<LO, HI>: every n of the range reaches f with N == n, exactly once; no n outside it reaches f at all
template <int LO, int HI>
static void check_count() {
  for (int n = LO - 3; n <= HI + 3; ++n) {
    int calls = 0, seen = -100;
    const int rc = pn::with_count<LO, HI>(n, [&](auto N) {
      static_assert(decltype(N)::value >= LO && decltype(N)::value <= HI, "instantiated outside the range");
      ++calls;
      seen = decltype(N)::value;
      return 40 + decltype(N)::value;          // what f returns comes back
    });
    if (n >= LO && n <= HI) CHECK(calls == 1 && seen == n && rc == 40 + n);
    else CHECK(calls == 0 && rc == pn::kNoCase);
  }
}

int main() {
  check_count<0, 7>();
  check_count<1, 7>();
  check_count<1, 8>();
  CHECK(pn::with_count<1, 7>(-2147483647 - 1, [](auto) { return 0; }) == pn::kNoCase);
  CHECK(pn::with_count<1, 7>(2147483647, [](auto) { return 0; }) == pn::kNoCase);

  // with_dtype: the element type of the dtype, nothing for any other value
  CHECK(pn::with_dtype(PN_F32, [](auto t) { return std::is_same<decltype(t), float>::value ? 4 : 0; }) == 4);
  CHECK(pn::with_dtype(PN_F64, [](auto t) { return std::is_same<decltype(t), double>::value ? 8 : 0; }) == 8);
  for (int dtype = -3; dtype <= 9; ++dtype) {
    if (dtype == PN_F32 || dtype == PN_F64) continue;
    int calls = 0;
    CHECK(pn::with_dtype(dtype, [&](auto) { return ++calls; }) == pn::kNoCase && calls == 0);
  }

  // with_width: 16 bytes of T, or one element
  auto width = [](auto W) { return (int)decltype(W)::value; };
  CHECK(pn::with_width<float>(true, width) == 4 && pn::with_width<float>(false, width) == 1);
  CHECK(pn::with_width<double>(true, width) == 2 && pn::with_width<double>(false, width) == 1);

  // blocks_for: rounded up, at least 1, at most the cap where there is one
  const int64_t per = 256;
  CHECK(pn::blocks_for(0, per) == 1 && pn::blocks_for(1, per) == 1);
  CHECK(pn::blocks_for(per, per) == 1 && pn::blocks_for(per + 1, per) == 2);
  CHECK(pn::blocks_for(0, per, 8) == 1 && pn::blocks_for(per + 1, per, 8) == 2);
  CHECK(pn::blocks_for(8 * per, per, 8) == 8 && pn::blocks_for(8 * per + 1, per, 8) == 8 && pn::blocks_for(7 * per + 1, per, 8) == 8);
  CHECK(pn::blocks_for(7 * per, per, 8) == 7 && pn::blocks_for(8 * per + 1, per, 0) == 9);
  CHECK(pn::blocks_for(((int64_t)1 << 40) + 1, per, 4096) == 4096 && pn::blocks_for(((int64_t)1 << 40) + 1, per) == ((int64_t)1 << 32) + 1);

  // aligned16: one pointer, several, a table; null counts as aligned
  alignas(16) static char buf[64];
  const void *tab[3] = {buf, buf + 16, buf + 32};
  CHECK(pn::aligned16(buf) && !pn::aligned16(buf + 8) && pn::aligned16(nullptr));
  CHECK(pn::aligned16(buf, buf + 16, buf + 48) && !pn::aligned16(buf, buf + 4, buf + 48) && !pn::aligned16(buf, buf + 16, buf + 1));
  CHECK(pn::aligned16(buf, (const void *)nullptr));
  CHECK(pn::aligned16(tab, 3) && pn::aligned16(tab, 0));
  tab[2] = buf + 40;
  CHECK(!pn::aligned16(tab, 3) && pn::aligned16(tab, 2));

  if (g_fail) return 1;
  std::printf("dispatch check ok\n");
  return 0;
}
