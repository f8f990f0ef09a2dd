// Stand-alone host program: the three per-view scratch size queries of the C ABI (mh_capture_scratch_bytes,
// mh_photo_scratch_bytes, mh_support_scratch_bytes) against the closed forms of include/mh_pmvo.h, written out here as
// literals, over a grid of sizes; and the arguments they answer 0 for.  The queries launch nothing, so this needs no GPU.
// Built and run by tests/test_scratch_sizes.py.
//   scratch_sizes_main <path of libmhpmvo.so>      one line per size (n H W ss capture photo support); exit status 1 on a mismatch
#include <dlfcn.h>

#include <cstddef>
#include <cstdio>

typedef size_t (*query3)(int, int, int);
typedef size_t (*query4)(int, int, int, int);

static size_t a256(size_t b) { return (b + 255) / 256 * 256; }

int main(int argc, char **argv) {
    void *lib = argc > 1 ? dlopen(argv[1], RTLD_NOW | RTLD_LOCAL) : nullptr;
    if (!lib) {
        fprintf(stderr, "cannot load the library: %s\n", argc > 1 ? dlerror() : "no path given");
        return 2;
    }
    const query3 capture = (query3)dlsym(lib, "mh_capture_scratch_bytes"), support = (query3)dlsym(lib, "mh_support_scratch_bytes");
    const query4 photo = (query4)dlsym(lib, "mh_photo_scratch_bytes");
    if (!capture || !support || !photo) {
        fprintf(stderr, "a size query is missing\n");
        return 2;
    }
    const int ns[] = {0, 1, 2, 255, 256, 257, 100000}, hw[][2] = {{1, 1}, {3, 5}, {1080, 1920}}, sss[] = {1, 2, 4, 8};
    int bad = 0;
    for (int n_points : ns)
        for (const auto &im : hw)
            for (int ss : sss) {
                const int H = im[0], W = im[1];
                // dropped 256 B | vert | valid | ..., the per-point regions sized for at least one point
                const size_t n = (size_t)(n_points > 0 ? n_points : 1), npix = (size_t)H * W, nsub = npix * ss * ss;
                const size_t want_capture = 256 + a256(n * 12) + a256(n) + 2 * a256(npix * 4) + 2 * a256(npix * 8);
                const size_t want_photo = 256 + a256(n * 12) + 2 * a256(n) + a256(nsub * 8);
                const size_t want_support = 256 + a256(n * 12) + a256(n) + a256(npix * 4);
                const size_t c = capture(n_points, H, W), p = photo(n_points, H, W, ss), s = support(n_points, H, W);
                printf("%d %d %d %d %zu %zu %zu\n", n_points, H, W, ss, c, p, s);
                if (c != want_capture || p != want_photo || s != want_support) {
                    fprintf(stderr, "n %d, %d x %d, ss %d: capture %zu (%zu), photo %zu (%zu), support %zu (%zu)\n", n_points, H,
                            W, ss, c, want_capture, p, want_photo, s, want_support);
                    ++bad;
                }
            }
    // what the queries refuse: negative n, an image of 2^31 pixels or more, no pixel, a supersampling factor that is none
    const size_t zeros[] = {capture(-1, 4, 4),       photo(-1, 4, 4, 1),       support(-1, 4, 4),
                            capture(1, 65536, 32768), photo(1, 65536, 32768, 1), support(1, 65536, 32768),
                            capture(1, 0, 4),         photo(1, 4, 0, 1),         support(1, 0, 4),
                            photo(1, 4, 4, 3),        photo(1, 4, 4, 0),         photo(1, 4, 4, 16),
                            photo(1, 32768, 32768, 2)};
    for (size_t i = 0; i < sizeof(zeros) / sizeof(zeros[0]); ++i)
        if (zeros[i] != 0) {
            fprintf(stderr, "refused case %zu answered %zu\n", i, zeros[i]);
            ++bad;
        }
    return bad ? 1 : 0;
}
