// Host-side check of mikudance_amd/csrc/latent_resize.hip, no GPU needed: the launcher's argument checks (every refusing path, nothing is ever
// launched) and the per-pixel arithmetic (resize_pixel is host-callable) run on the CPU, so that they can run under the host sanitizers.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -I mikudance_amd/csrc tools/latent_resize_host_check.cpp -o /tmp/latent_resize_host_check
//   /tmp/latent_resize_host_check refuse                                   every refusal: status -1, a message, exit code 0 when all are as expected
//   /tmp/latent_resize_host_check resize F Hi Wi Ho Wo mode in.f16 out.f16 the kernel's arithmetic on a raw little-endian fp16 file (tests/hires_ref.py
//                                                                          holds the reference to compare out.f16 with)
#include "latent_resize.hip"

#include <stdarg.h>
#include <string.h>

#include <vector>

static char g_err[512];
void md_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

static int refuse() {
  alignas(16) static half_t a[64], b[64];
  void *x = a, *y = b;
  struct {
    const char* what;
    const void* x;
    void* y;
    int F, Hi, Wi, Ho, Wo, mode;
  } cases[] = {{"NULL x", nullptr, y, 1, 2, 2, 2, 2, 1},
               {"NULL y", x, nullptr, 1, 2, 2, 2, 2, 1},
               {"misaligned x", (char*)x + 2, y, 1, 2, 2, 2, 2, 1},
               {"misaligned y", x, (char*)y + 4, 1, 2, 2, 2, 2, 1},
               {"F = 0", x, y, 0, 2, 2, 2, 2, 1},
               {"Hi < 0", x, y, 1, -2, 2, 2, 2, 1},
               {"Wi = 0", x, y, 1, 2, 0, 2, 2, 1},
               {"Ho = 0", x, y, 1, 2, 2, 0, 2, 1},
               {"Wo < 0", x, y, 1, 2, 2, 2, -1, 1},
               {"mode 3", x, y, 1, 2, 2, 2, 2, 3},
               {"mode -1", x, y, 1, 2, 2, 2, 2, -1},
               {"input beyond int", x, y, 2, 46341, 46341, 2, 2, 1},
               {"output beyond int", x, y, 2, 2, 2, 46341, 46341, 1},
               {"input far beyond long", x, y, INT_MAX, INT_MAX, INT_MAX, 2, 2, 2},
               {"output far beyond long", x, y, INT_MAX, 2, 2, INT_MAX, INT_MAX, 0},
               {"y aliases x", x, x, 1, 2, 2, 2, 2, 1},
               {"y overlaps x", x, (char*)x + 8, 1, 2, 2, 2, 2, 2}};
  int bad = 0;
  for (auto& c : cases) {
    g_err[0] = 0;
    const int rc = md_latent_resize_f16(c.x, c.y, c.F, c.Hi, c.Wi, c.Ho, c.Wo, c.mode, nullptr);
    const bool ok = rc == MD_ERR_ARG && strncmp(g_err, "md_latent_resize_f16", 20) == 0;
    printf("%-24s -> %d  %s%s\n", c.what, rc, g_err, ok ? "" : "   UNEXPECTED");
    bad += !ok;
  }
  return bad;
}

template <int MODE>
static void run(const half_t* x, half_t* y, long total, int Hi, int Wi, int Ho, int Wo) {
  for (long i = 0; i < total; ++i) resize_pixel<MODE>(x, y, i, Hi, Wi, Ho, Wo);
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "refuse")) return refuse() ? 1 : 0;
  if (argc != 10 || strcmp(argv[1], "resize")) {
    fprintf(stderr, "usage: %s refuse | resize F Hi Wi Ho Wo mode in.f16 out.f16\n", argv[0]);
    return 2;
  }
  const int F = atoi(argv[2]), Hi = atoi(argv[3]), Wi = atoi(argv[4]), Ho = atoi(argv[5]), Wo = atoi(argv[6]), mode = atoi(argv[7]);
  if (F < 1 || Hi < 1 || Wi < 1 || Ho < 1 || Wo < 1 || mode < 0 || mode > 2 || (long)F * Hi * Wi > (1L << 26) || (long)F * Ho * Wo > (1L << 26)) return 2;
  std::vector<half_t> x((size_t)F * Hi * Wi * 4), y((size_t)F * Ho * Wo * 4);      // exact sizes: an index outside them is a sanitizer report
  FILE* fi = fopen(argv[8], "rb");
  if (!fi || fread(x.data(), 2, x.size(), fi) != x.size()) return 3;
  fclose(fi);
  const long total = (long)F * Ho * Wo;
  if (mode == 0)
    run<0>(x.data(), y.data(), total, Hi, Wi, Ho, Wo);
  else if (mode == 1)
    run<1>(x.data(), y.data(), total, Hi, Wi, Ho, Wo);
  else
    run<2>(x.data(), y.data(), total, Hi, Wi, Ho, Wo);
  FILE* fo = fopen(argv[9], "wb");
  if (!fo || fwrite(y.data(), 2, y.size(), fo) != y.size()) return 3;
  fclose(fo);
  return 0;
}
