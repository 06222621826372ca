// Stand-alone host check of csrc/device_mem.hpp (DevMem, DevPool) against tests/fake_hip: every ownership rule
// the plans and host entry points rely on, on success and with each allocation failing in turn.  Leaks are
// asserted on the fake's live-allocation count; built with -fsanitize=address,undefined by
// tests/test_device_mem_host.py.  Exits non-zero at the first violated rule.
#include <cstdarg>
#include <cstdio>
#include <utility>

#include "device_mem.hpp"

namespace sg {
void set_error(const char *, ...) {}
int fail(int code, const char *, ...) { return code; }
}  // namespace sg

using sg::DevMem;
using sg::DevPool;

static int g_bad = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_bad;                                                      \
        }                                                                 \
    } while (0)

static void test_devmem() {
    {
        DevMem m;
        CHECK(m.bytes() == 0 && m.at() == nullptr);
        CHECK(m.ensure(100) == SG_OK && m.bytes() == 100 && m.at() && fake_live == 1);
        void *p = m.at();
        CHECK(m.ensure(40) == SG_OK && m.at() == p && m.bytes() == 100);   // smaller: kept
        CHECK(m.ensure(100) == SG_OK && m.at() == p && m.bytes() == 100);  // equal: kept
        CHECK(m.at<char>(8) == (char *)p + 8);
        CHECK(m.ensure(101) == SG_OK && m.bytes() == 101 && fake_live == 1);  // larger: replaced, exact size
        m.at<char>()[100] = 1;  // (the sanitizer checks the new size)
        fake_fail_in = 1;
        CHECK(m.ensure(500) == SG_ERR_NOMEM && m.bytes() == 0 && m.at() == nullptr && fake_live == 0);
        CHECK(m.ensure(50) == SG_OK && m.bytes() == 50 && fake_live == 1);  // the next call tries again
        p = m.at();
        DevMem n(std::move(m));  // move-construct
        CHECK(m.bytes() == 0 && m.at() == nullptr && n.at() == p && n.bytes() == 50 && fake_live == 1);
        DevMem o;
        CHECK(o.ensure(7) == SG_OK && fake_live == 2);
        o = std::move(n);  // move-assign frees the target's own buffer
        CHECK(n.bytes() == 0 && n.at() == nullptr && o.at() == p && o.bytes() == 50 && fake_live == 1);
        o.reset();
        CHECK(o.bytes() == 0 && o.at() == nullptr && fake_live == 0);
        CHECK(o.ensure(9) == SG_OK && fake_live == 1);
    }
    CHECK(fake_live == 0);  // scope exit frees
}

struct Owner {  // a plan in miniature: slots of several types
    int32_t *a = nullptr;
    double *b = nullptr;
    void *c = nullptr;
    uint16_t *d = nullptr;
    bool all_null() const { return !a && !b && !c && !d; }
};

// n = 4 allocations in a fixed order, as the ensure_* functions and table builders make them
static int fill(DevPool &pool, Owner &o) {
    SG_TRY(pool.alloc(&o.a, 64));
    SG_TRY(pool.upload(&o.b, std::vector<double>{1.0, 2.0, 3.0}));
    SG_TRY(pool.alloc(&o.c, 0));
    SG_TRY(pool.upload(&o.d, std::vector<uint16_t>()));
    return SG_OK;
}

static void test_devpool() {
    {
        Owner o;
        DevPool pool;
        CHECK(fill(pool, o) == SG_OK && fake_live == 4);
        CHECK(o.a && o.b && o.c && o.d);  // (an empty upload and a zero-byte alloc still give a slot)
        CHECK(o.b[0] == 1.0 && o.b[2] == 3.0);
        pool.release();
        CHECK(o.all_null() && fake_live == 0);
        pool.release();  // no-op
        CHECK(o.all_null() && fake_live == 0);
        CHECK(fill(pool, o) == SG_OK && fake_live == 4 && o.a && o.d);  // alloc after release
        pool.release();
        CHECK(fake_live == 0);
    }
    for (int k = 1; k <= 4; ++k) {  // the k-th of the 4 allocations fails
        Owner o;
        DevPool pool;
        fake_fail_in = k;
        CHECK(fill(pool, o) == SG_ERR_NOMEM);
        CHECK(fake_live == k - 1);  // what was allocated before stays owned
        pool.release();
        CHECK(o.all_null() && fake_live == 0);
        CHECK(fill(pool, o) == SG_OK && fake_live == 4);  // and the pool is usable again
    }  // (destruction without release frees)
    CHECK(fake_live == 0);
    {
        Owner o;
        DevPool pool;
        CHECK(fill(pool, o) == SG_OK && fake_live == 4);
    }
    CHECK(fake_live == 0);
}

// The shape of sg_section_softmax and the other host shims: local scratch, then checked calls that return early
static int shim(hipError_t later) {
    DevMem mem;
    SG_TRY(mem.ensure(256));
    SG_HIP(later);
    return SG_OK;
}

static void test_early_return() {
    CHECK(shim(hipErrorInvalidValue) == SG_ERR_HIP && fake_live == 0);
    CHECK(shim(hipErrorOutOfMemory) == SG_ERR_NOMEM && fake_live == 0);
    CHECK(shim(hipSuccess) == SG_OK && fake_live == 0);
    fake_fail_in = 1;
    CHECK(shim(hipSuccess) == SG_ERR_NOMEM && fake_live == 0);
}

int main() {
    test_devmem();
    test_devpool();
    test_early_return();
    if (g_bad) std::fprintf(stderr, "%d check(s) failed\n", g_bad);
    else std::printf("device_mem: ok\n");
    return g_bad ? 1 : 0;
}
