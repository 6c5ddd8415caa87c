// The bucket and work-list arithmetic of csrc/wk_weigh_wide.hpp on the CPU: wide_bucket against a plain division with
// the clamp, and wide_plan against what the histogram and the merge rely on -- every bucket's records are one range of
// the second buffer, the ranges start at multiples of 4 words, do not overlap and fit wide_room; a bucket has items
// iff it has records; the teams of a bucket cover its tiles; the items are at most n_wg + (non-empty buckets) and
// every item names the bucket whose [item_first[k], item_first[k + 1]) holds it.  A program of its own, built with
// -fsanitize=address,undefined by tests/test_weigh_wide_host.py: nothing is loaded into python.
#include <cstdint>
#include <cstdio>
#include <memory>
#include <random>
#include <vector>

#include "wk_weigh_wide.hpp"

using namespace wk;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (++failures <= 20) printf("line %d: %s\n", __LINE__, #cond);  \
        }                                                                    \
    } while (0)

static void check_plan(const std::vector<uint32_t>& counts, uint32_t n_wg) {
    const uint32_t nb = (uint32_t)counts.size();
    // (the plan on the heap, exactly its size: a store past an array is seen)
    std::unique_ptr<WidePlan> p(new WidePlan);
    wide_plan(counts.data(), nb, n_wg, p.get());
    uint64_t total = 0;
    uint32_t nonempty = 0, longest = 0;
    for (uint32_t c : counts) {
        total += c;
        nonempty += c ? 1u : 0u;
    }
    CHECK(p->n_buckets == nb);
    CHECK(p->n_items <= n_wg + nonempty);
    CHECK(p->n_items <= kWideMaxItems);
    CHECK(p->n_items >= nonempty);
    CHECK(p->item_first[0] == 0 && p->item_first[nb] == p->n_items);
    CHECK(p->start[0] == 0);
    CHECK((uint64_t)p->start[nb] <= wide_room(total));
    const uint64_t fair = (total + n_wg - 1) / n_wg;
    for (uint32_t k = 0; k < nb; ++k) {
        CHECK(p->count[k] == counts[k]);
        CHECK(p->start[k] % kWideAlign == 0);
        CHECK(p->start[k + 1] >= p->start[k] + counts[k]);
        CHECK(p->start[k + 1] < p->start[k] + counts[k] + kWideAlign);
        CHECK(p->item_first[k + 1] >= p->item_first[k]);
        const uint32_t teams = p->item_first[k + 1] - p->item_first[k];
        CHECK((teams > 0) == (counts[k] > 0));
        if (teams) {  // no team walks more than a workgroup's fair share
            const uint64_t share = ((uint64_t)counts[k] + teams - 1) / teams;
            CHECK(share <= (fair ? fair : 1));
            if (share > longest) longest = (uint32_t)share;
        }
        for (uint32_t i = p->item_first[k]; i < p->item_first[k + 1]; ++i) CHECK(p->item_bucket[i] == k);
    }
    (void)longest;
}

int main() {
    // buckets: seams, the clamp, bits above the subject field
    CHECK(kWideMaxBuckets == 207);
    const uint32_t seams[] = {0u, kWideBins - 1u, kWideBins, 32u * kWideBins - 1u, 32u * kWideBins, 206u * kWideBins - 1u, 206u * kWideBins, (1u << 23) - 1u};
    for (uint32_t s : seams)
        for (uint32_t nb : {1u, 2u, 33u, 34u, 207u})
            for (uint32_t high : {0u, 1u << 23, 0xFF800000u}) {
                const uint32_t plain = s / kWideBins;
                CHECK(wide_bucket(s | high, nb) == (plain < nb ? plain : nb - 1u));
            }
    std::mt19937 rng(7);
    for (int i = 0; i < 200000; ++i) {
        const uint32_t w = rng(), nb = 1u + rng() % kWideMaxBuckets;
        const uint32_t plain = (w & 0x7FFFFFu) / kWideBins;
        CHECK(wide_bucket(w, nb) == (plain < nb ? plain : nb - 1u));
    }
    // plans
    for (uint32_t n_wg : {1u, 8u, 255u, 256u, 304u, kWideMaxWgs}) {
        check_plan(std::vector<uint32_t>(1, 0u), n_wg);
        check_plan(std::vector<uint32_t>(1, 1u), n_wg);
        check_plan(std::vector<uint32_t>(kWideMaxBuckets, 0u), n_wg);
        check_plan(std::vector<uint32_t>(kWideMaxBuckets, 1u), n_wg);
        check_plan(std::vector<uint32_t>(kWideMaxBuckets, 5186u), n_wg);           // (207 x 5186 < 2^30)
        {
            std::vector<uint32_t> one(kWideMaxBuckets, 0u);
            one[150] = (1u << 30) - 1u;                                          // the most records a flush holds
            check_plan(one, n_wg);
            one[150] = 100000u;
            check_plan(one, n_wg);
        }
        {
            std::vector<uint32_t> zipf(kWideMaxBuckets);
            for (uint32_t k = 0; k < kWideMaxBuckets; ++k) zipf[k] = 900000000u / ((k + 1u) * 6u);
            check_plan(zipf, n_wg);
            std::vector<uint32_t> tail(zipf.rbegin(), zipf.rend());
            check_plan(tail, n_wg);
        }
        for (int i = 0; i < 300; ++i) {
            const uint32_t nb = 1u + rng() % kWideMaxBuckets;
            std::vector<uint32_t> c(nb);
            const uint32_t cap = 1u << (rng() % 22);
            for (uint32_t& x : c) x = (rng() % 3u) ? rng() % cap : 0u;
            check_plan(c, n_wg);
        }
    }
    printf("weigh_wide_host: %d failures\n", failures);
    return failures ? 1 : 0;
}
