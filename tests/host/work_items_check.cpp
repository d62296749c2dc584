// work_items_check.cpp — the work-item contract (tinyrenderder_amd/csrc/work_items.h) on the host: every item of a list is taken by
// exactly one workgroup of the raster launch, and the item word survives encode / decode.  tests/test_work_items.py compiles and runs it.
#include <cstdio>
#include <vector>
#include "work_items.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

int main() {
    // ---- every item is taken exactly once ----
    const uint32_t Gs[] = { 0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 8191 };
    int launches = 0;
    for (uint32_t G : Gs) {
        const uint32_t caps[] = { G, G + 5, 4 * G };
        for (uint32_t cap : caps) {
            const uint32_t max_items = cap < 1 ? 1 : cap;
            const uint32_t grid = trgl_item_grid(max_items);
            CHECK(grid >= max_items && grid % 8 == 0 && grid < max_items + 8, "G %u max_items %u: grid %u", G, max_items, grid);
            std::vector<uint32_t> taken(G, 0);
            for (uint32_t b = 0; b < grid; ++b) {
                uint32_t g = 0xffffffffu;
                if (!trgl_item_of_workgroup(b, G, &g)) continue;
                CHECK(g < G, "G %u max_items %u: workgroup %u yields item %u", G, max_items, b, g);
                if (g < G) ++taken[g];
                // the mapping, written out: an eighth of the list per value of b mod 8
                const uint32_t per = (G + 7) / 8;
                CHECK(g == (b & 7) * per + (b >> 3) && (b >> 3) < per, "G %u: workgroup %u -> %u", G, b, g);
            }
            for (uint32_t g = 0; g < G; ++g) CHECK(taken[g] == 1, "G %u max_items %u: item %u taken %u times", G, max_items, g, taken[g]);
            ++launches;
        }
    }
    // ---- the item word ----
    const uint32_t tiles[] = { 0, 1, (1u << 24) - 1 };
    for (uint32_t t : tiles) {
        for (uint32_t r = 0; r < 4; ++r) {
            const uint32_t item = trgl_item_rows(t, r);
            CHECK(trgl_item_tile(item) == t && trgl_item_brow(item) == r && !(item & TRGL_ITEM_CLEAR), "tile %u row %u -> %08x", t, r, item);
            // the flag on top of a row item keeps tile and row
            const uint32_t flagged = item | TRGL_ITEM_CLEAR;
            CHECK(trgl_item_tile(flagged) == t && trgl_item_brow(flagged) == r && (flagged & TRGL_ITEM_CLEAR), "flagged %08x", flagged);
        }
        const uint32_t c = trgl_item_clear(t);
        CHECK((c & TRGL_ITEM_CLEAR) && trgl_item_tile(c) == t && trgl_item_brow(c) == 0, "clear item of tile %u -> %08x", t, c);
    }
    // ---- the partial ----
    CHECK(TRGL_ITEM_STATS_WORDS == 4 && TRGL_ITEM_FRAGS == 0 && TRGL_ITEM_KMIN == 1 && TRGL_ITEM_KMAX == 2, "layout of a partial");
    CHECK(TRGL_ITEM_KMIN_NONE == ~0ull && TRGL_ITEM_KMAX_NONE == 0ull, "neutral keys");
    CHECK(zkey(-__builtin_inf()) > TRGL_ITEM_KMAX_NONE && zkey(__builtin_inf()) < TRGL_ITEM_KMIN_NONE, "neutral keys lie outside every depth's key");
    std::printf("%d launches checked, %d failures\n", launches, failures);
    return failures ? 1 : 0;
}
