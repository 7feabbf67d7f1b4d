// request_shapes.cpp -- the HIP-free part of the request scaffold (csrc/dt_request_shape.hpp) under
// AddressSanitizer + UndefinedBehaviorSanitizer: the request validator, the LV packer and
// FrontierSet::read over every shape the per-request calls meet.  Each vector is sized exactly, so
// an index one past a request, an LV set or a frontier is a sanitizer report.
// Prints "shapes ok <checks>" and exits 0; a failed check names its line and exits 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dt_request_shape.hpp"

using namespace dtgpu;

static int checks = 0;
#define CHECK(x) do { checks++; if (!(x)) { fprintf(stderr, "request_shapes.cpp:%d: %s\n", __LINE__, #x); exit(1); } } while (0)

struct Desc {   // the two fields of a HistDesc / SumDesc the packer writes
    uint32_t before = 7;
    uint64_t req_off = 99;
    uint32_t n_req = 99, after = 7;
};

// One request of k LVs whose CSR starts at `start`: valid, and packed from 0.
static void one_request(size_t k, size_t start) {
    std::vector<uint64_t> lv(start + k);
    for (size_t j = 0; j < k; j++) lv[start + j] = 1000 + j;
    const std::vector<size_t> off = {start, start + k};
    const uint32_t doc = 0;
    CHECK(request_ok(true, 1, &doc, lv.data(), off.data(), 1));
    CHECK(request_ok(true, 1, &doc, nullptr, off.data(), 1) == (k == 0));   // no LVs: no LV array needed
    std::vector<uint32_t> req;
    Desc d;
    pack_sets(lv.data(), off.data(), 1, req, &d, &Desc::req_off, &Desc::n_req);
    CHECK(req.size() == k && d.req_off == 0 && d.n_req == k && d.before == 7 && d.after == 7);
    for (size_t j = 0; j < k; j++) CHECK(req[j] == 1000 + j);
}

int main() {
    // an empty batch: nothing is read, not even null arrays
    CHECK(request_ok(true, 0, nullptr, nullptr, nullptr, 0));
    CHECK(!request_ok(false, 0, nullptr, nullptr, nullptr, 0));   // the base's arrays must exist all the same
    {
        std::vector<uint32_t> req(3, 5);
        pack_sets<Desc>(nullptr, nullptr, 0, req, nullptr, &Desc::req_off, &Desc::n_req);
        CHECK(req.empty());
        FrontierSet fs;
        fs.assign(0);
        size_t k = 42;
        CHECK(fs.read(0, nullptr, 0, &k) == DTGPU_ERR_ARG && k == 42);
    }
    // one request of 0, 1, 64 and 65 LVs, from offset 0 and from a CSR that starts elsewhere
    for (size_t k : {size_t(0), size_t(1), size_t(64), size_t(65)})
        for (size_t start : {size_t(0), size_t(3)}) one_request(k, start);
    {   // three requests, the middle one empty, offsets from 2: req_off counts from the first set
        const std::vector<uint64_t> lv = {9, 9, 10, 11, (1ull << 32) + 5, 0xFFFFFFFFull, 0xFFFFFFFEull};
        const std::vector<size_t> off = {2, 4, 4, 7};
        const std::vector<uint32_t> doc = {1, 0, 1};
        CHECK(request_ok(true, 2, doc.data(), lv.data(), off.data(), 3));
        std::vector<uint32_t> req;
        std::vector<Desc> d(3);
        pack_sets(lv.data(), off.data(), 3, req, d.data(), &Desc::req_off, &Desc::n_req);
        CHECK(req.size() == 5);
        CHECK(d[0].req_off == 0 && d[0].n_req == 2 && d[1].req_off == 2 && d[1].n_req == 0 && d[2].req_off == 2 && d[2].n_req == 3);
        // an LV above 2^32 clamps to 0xFFFFFFFF, the largest 32-bit ones stay
        CHECK(req[0] == 10 && req[1] == 11 && req[2] == 0xFFFFFFFFu && req[3] == 0xFFFFFFFFu && req[4] == 0xFFFFFFFEu);
        CHECK(lv32(1ull << 32) == 0xFFFFFFFFu && lv32(~0ull) == 0xFFFFFFFFu && lv32(0) == 0);
        // the validator's rejections
        CHECK(!request_ok(false, 2, doc.data(), lv.data(), off.data(), 3));   // base not decoded
        CHECK(!request_ok(true, 1, doc.data(), lv.data(), off.data(), 3));    // doc[i] == base_n
        CHECK(!request_ok(true, 2, nullptr, lv.data(), off.data(), 3));
        CHECK(!request_ok(true, 2, doc.data(), lv.data(), nullptr, 3));
        CHECK(!request_ok(true, 2, doc.data(), nullptr, off.data(), 3));      // LVs named, none given
        const std::vector<size_t> down = {2, 4, 3, 7}, first_down = {4, 2, 4, 7}, none = {6, 6, 6, 6};
        CHECK(!sets_ok(lv.data(), down.data(), 3) && !sets_ok(lv.data(), first_down.data(), 3));
        CHECK(request_ok(true, 2, doc.data(), nullptr, none.data(), 3));      // every set empty: no LV array needed
    }
    {   // FrontierSet::read
        FrontierSet fs;
        fs.assign(3);
        CHECK(fs.status.size() == 3 && fs.n_front.size() == 3);
        for (size_t j = 0; j < 3 * DECODE_MAX_FRONTIER; j++) fs.front[j] = uint32_t(100 * (j / DECODE_MAX_FRONTIER) + j % DECODE_MAX_FRONTIER);
        fs.front[DECODE_MAX_FRONTIER] = 0xFFFFFFFFu;
        fs.n_front = {2, DECODE_MAX_FRONTIER, 0};
        fs.status = {0, 0, 66};   // a failed request: the producer left it no frontier
        size_t k = 42;
        CHECK(fs.read(0, nullptr, 0, &k) == DTGPU_OK && k == 2);   // cap 0: the width only
        std::vector<uint64_t> one(1, 77);
        k = 42;
        CHECK(fs.read(0, one.data(), 1, &k) == DTGPU_OK && k == 2 && one[0] == 0);   // cap below the width
        std::vector<uint64_t> two(2, 77);
        CHECK(fs.read(0, two.data(), 2, nullptr) == DTGPU_OK && two[0] == 0 && two[1] == 1);   // cap equal to it
        std::vector<uint64_t> wide(DECODE_MAX_FRONTIER, 77);
        k = 42;
        CHECK(fs.read(1, wide.data(), wide.size(), &k) == DTGPU_OK && k == DECODE_MAX_FRONTIER);
        CHECK(wide[0] == 0xFFFFFFFFull && wide[1] == 101 && wide[DECODE_MAX_FRONTIER - 1] == 100 + DECODE_MAX_FRONTIER - 1);
        std::vector<uint64_t> big(DECODE_MAX_FRONTIER + 4, 77);   // a cap above the width writes the width only
        CHECK(fs.read(1, big.data(), big.size(), nullptr) == DTGPU_OK && big[DECODE_MAX_FRONTIER] == 77);
        k = 42;
        CHECK(fs.read(2, two.data(), 2, &k) == dtgpu_status(66) && k == 0 && two[0] == 0);   // status, no frontier
        k = 42;
        CHECK(fs.read(3, two.data(), 2, &k) == DTGPU_ERR_ARG && k == 42);
        CHECK(fs.read(0, nullptr, 1, &k) == DTGPU_ERR_ARG && k == 42);
    }
    printf("shapes ok %d\n", checks);
    return 0;
}
