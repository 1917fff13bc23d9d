// owned.cpp - csrc/mc_owned.h on the CPU (tests/test_owned_host.py): the owners over a fake of the eight runtime calls that make and
// destroy device buffers, pinned buffers, streams and events.  The fake keeps each resource in malloc'd memory (so ASan sees a leak
// or a double free), logs every call in order, and can fail the k-th creation.  Prints one "ok <case>" line per case that held;
// exit status 1 with the first failed check otherwise.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

// ---- the fake runtime ---------------------------------------------------------------------------------------------------------------
enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };
struct FakeStream; struct FakeEvent;
typedef FakeStream *hipStream_t;
typedef FakeEvent *hipEvent_t;
enum { hipHostMallocDefault = 0, hipEventDisableTiming = 2 };
static const char *hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "out of memory"; }
static thread_local std::string g_err;

struct Call { char op; void *p; };                                 // op: D/P/S/E made, d/p/s/e destroyed
static std::vector<Call> g_log;
static int g_made = 0, g_fail_at = 0;                              // creations so far; the creation that fails (1-based, 0: none)
static int g_notiming = 0;                                         // events made with hipEventDisableTiming

static hipError_t fake_make(char op, void **out, size_t bytes)
{
    *out = nullptr;
    if (++g_made == g_fail_at) return hipErrorOutOfMemory;
    if (bytes == 0) return hipSuccess;                             // (hipMalloc of nothing: success and a null pointer)
    *out = malloc(bytes);
    g_log.push_back({op, *out});
    return hipSuccess;
}
static hipError_t fake_kill(char op, void *p) { g_log.push_back({op, p}); free(p); return hipSuccess; }

static hipError_t hipMalloc(void **p, size_t n) { return fake_make('D', p, n); }
static hipError_t hipFree(void *p) { return fake_kill('d', p); }
static hipError_t hipHostMalloc(void **p, size_t n, unsigned) { return fake_make('P', p, n); }
static hipError_t hipHostFree(void *p) { return fake_kill('p', p); }
static hipError_t hipStreamCreate(hipStream_t *s) { return fake_make('S', (void **)s, 8); }
static hipError_t hipStreamDestroy(hipStream_t s) { return fake_kill('s', s); }
static hipError_t hipEventCreate(hipEvent_t *e) { return fake_make('E', (void **)e, 8); }
static hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned flags) { if (flags == hipEventDisableTiming) g_notiming++; return fake_make('E', (void **)e, 8); }
static hipError_t hipEventDestroy(hipEvent_t e) { return fake_kill('e', e); }

#include "../../microbecensus_amd/csrc/mc_owned.h"

// ---- the checks ---------------------------------------------------------------------------------------------------------------------
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s: check failed: %s\n", __FILE__, __LINE__, g_case.c_str(), #cond); exit(1); } } while (0)
static std::string g_case;

static bool all_dead() { for (int k = 0; k < MC_LIVE_N; k++) if (mc_live[k].load() != 0) return false; return true; }
static int64_t live(int kind) { return mc_live[kind].load(); }
static void begin(const std::string &name) { g_case = name; g_log.clear(); g_made = 0; g_fail_at = 0; CHECK(all_dead()); }
static void end()
{
    CHECK(all_dead());
    size_t made = 0, killed = 0;                                     // every resource made was destroyed exactly once
    for (const Call &c : g_log) (c.op >= 'A' && c.op <= 'Z' ? made : killed)++;
    CHECK(made == killed);
    printf("ok %s\n", g_case.c_str());
}
// the log reads as the string of its ops
static std::string ops() { std::string s; for (const Call &c : g_log) s += c.op; return s; }

// O: the owner, make(o): its creating call, kind: its live count, M / m: its letters in the log
template <class O, class Make> static void owner_cases(const char *name, int kind, char M, char m, Make make)
{
    const std::string mk(1, M), kl(1, m);
    begin(std::string(name) + ": create, destroy");
    {
        O o;
        CHECK(!o && live(kind) == 0);
        CHECK(make(o) == 0 && o && live(kind) == 1);
    }
    CHECK(ops() == mk + kl && g_log[0].p == g_log[1].p);
    end();

    begin(std::string(name) + ": a second creation frees the first one first");
    {
        O o;
        CHECK(make(o) == 0);
        void *first = (void *)o.get();
        CHECK(make(o) == 0 && live(kind) == 1);
        CHECK(ops() == mk + kl + mk && g_log[1].p == first);         // (made, FREED, made: never two at once)
    }
    CHECK(ops() == mk + kl + mk + kl);
    end();

    begin(std::string(name) + ": move-construct");
    {
        O a;
        CHECK(make(a) == 0);
        void *pa = (void *)a.get();
        O b(std::move(a));
        CHECK(!a && (void *)b.get() == pa && live(kind) == 1 && ops() == mk);
    }
    CHECK(ops() == mk + kl);
    end();

    begin(std::string(name) + ": move-assign onto a full owner");
    {
        O a, b;
        CHECK(make(a) == 0 && make(b) == 0 && live(kind) == 2);
        void *pa = (void *)a.get(), *pb = (void *)b.get();
        b = std::move(a);
        CHECK(!a && (void *)b.get() == pa && live(kind) == 1);
        CHECK(ops() == mk + mk + kl && g_log[2].p == pb);            // the target's old resource, once
        O &self = b;
        b = std::move(self);                                         // (onto itself: nothing happens)
        CHECK((void *)b.get() == pa && live(kind) == 1 && ops() == mk + mk + kl);
    }
    CHECK(ops() == mk + mk + kl + kl);
    end();

    begin(std::string(name) + ": reset twice");
    {
        O o;
        CHECK(make(o) == 0);
        o.reset();
        CHECK(!o && live(kind) == 0 && ops() == mk + kl);
        o.reset();
        CHECK(!o && live(kind) == 0 && ops() == mk + kl);
    }
    CHECK(ops() == mk + kl);
    end();

    begin(std::string(name) + ": a failed creation leaves the owner empty and the error named");
    {
        O o;
        CHECK(make(o) == 0);
        g_fail_at = g_made + 1; g_err.clear();
        CHECK(make(o) == -1 && !o && live(kind) == 0);
        CHECK(g_err.find(": out of memory") != std::string::npos && g_err.compare(0, 3, "hip") == 0);
        CHECK(ops() == mk + kl);
    }
    CHECK(ops() == mk + kl);
    end();
}

int main()
{
    owner_cases<McDev<int>>("device buffer", MC_LIVE_DEV, 'D', 'd', [](McDev<int> &o) { return o.alloc(5); });
    owner_cases<McPin<double>>("pinned buffer", MC_LIVE_PIN, 'P', 'p', [](McPin<double> &o) { return o.alloc(3); });
    owner_cases<McStream>("stream", MC_LIVE_STREAM, 'S', 's', [](McStream &o) { return o.create(); });
    owner_cases<McEvent>("event", MC_LIVE_EVENT, 'E', 'e', [](McEvent &o) { return o.create(); });
    g_notiming = 0;
    owner_cases<McEvent>("event without timing", MC_LIVE_EVENT, 'E', 'e', [](McEvent &o) { return o.create(false); });
    g_case = "event without timing"; CHECK(g_notiming > 0);

    begin("device buffer: usable as the pointer it holds");
    {
        McDev<int> d;
        CHECK(d.alloc(4) == 0);
        int *p = d;
        for (int i = 0; i < 4; i++) d[i] = i * i;
        CHECK(p[3] == 9 && *(d + 2) == 4 && (void *)(d + 1) == (void *)(p + 1));
        McDev<int> none;
        CHECK(none.alloc(0) == 0 && !none && live(MC_LIVE_DEV) == 1); // (nothing asked for: nothing held, nothing counted)
    }
    end();

    begin("McDevBuf: five buffers, the third fails");
    {
        McDevBuf B;
        int *a = nullptr; double *b = nullptr; char *c = nullptr, *d = nullptr, *e = nullptr;
        g_fail_at = 3;
        const bool failed = B.get(&a, 10) || B.get(&b, 0) || B.get(&c, 7) || B.get(&d, 7) || B.get(&e, 7);   // (0 elements: one is made)
        CHECK(failed && a && b && !c && !d && !e && live(MC_LIVE_DEV) == 2 && ops() == "DD");
        CHECK(g_err.find("hipMalloc") == 0 && g_err.find(": out of memory") != std::string::npos);
    }
    CHECK(ops() == "DDdd" && ((g_log[2].p == g_log[0].p && g_log[3].p == g_log[1].p) || (g_log[2].p == g_log[1].p && g_log[3].p == g_log[0].p)));
    end();

    begin("McDevBuf: five buffers");
    {
        McDevBuf B;
        int *p[5] = {};
        for (int k = 0; k < 5; k++) CHECK(B.get(&p[k], (size_t)k + 1) == 0 && p[k]);
        CHECK(live(MC_LIVE_DEV) == 5);
    }
    CHECK(ops() == "DDDDDddddd");
    end();

    begin("McEvents: four events, the third fails");
    {
        McEvents ev;
        g_fail_at = 3;
        CHECK(ev.make(4) == -1 && live(MC_LIVE_EVENT) == 2 && g_err == "hipEventCreate failed");
        CHECK(ev[0] && ev[1] && ev[0] != ev[1]);
    }
    CHECK(ops() == "EEee");
    end();

    begin("every kind at once");
    {
        McDev<char> d; McPin<char> p; McStream s; McEvent e; McDevBuf B; McEvents ev; char *x = nullptr;
        CHECK(d.alloc(1) == 0 && p.alloc(1) == 0 && s.create() == 0 && e.create() == 0 && B.get(&x, 1) == 0 && ev.make(2) == 0);
        CHECK(live(MC_LIVE_DEV) == 2 && live(MC_LIVE_PIN) == 1 && live(MC_LIVE_STREAM) == 1 && live(MC_LIVE_EVENT) == 3);
    }
    end();
    return 0;
}
