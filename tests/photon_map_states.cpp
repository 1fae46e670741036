// Walks every transition of GlobalPhotons (raytracing_folder_amd/csrc/rt_photon_map.h), the record of whose the global photon map
// of a scene is and where it lies, on the CPU: the header alone, devices as fake addresses, the two device copies of
// rt_photons.cpp played by fetch().  After each step: the invariant, count(), serves() and source_on().  Exit status 0 and
// "ok" when everything held; tests/test_host.py compiles and runs it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../raytracing_folder_amd/csrc/rt_photon_map.h"

static int g_step = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "step %d, line %d: %s\n", g_step, __LINE__, #cond); exit(1); } } while (0)

static DeviceState *fake_device(int k) { static char dev[4]; return (DeviceState *)&dev[k]; }

// what holds after every step: `n` photons, whether the map serves the parameters (count 100, bounce 8, seed 5) and (100, 8, 6),
// and on which of the two devices it answers, with which buffer
static void expect(const GlobalPhotons &g, uint32_t n, bool generated, bool serves5, bool serves6, const rt_photon *on_a, const rt_photon *on_b)
{
    g_step++;
    CHECK(g.invariant());
    CHECK(g.count() == n);
    CHECK(g.is_generated() == generated);
    CHECK(g.serves(100, 8, 5) == serves5);
    CHECK(g.serves(100, 8, 6) == serves6);
    CHECK(!g.serves(101, 8, 5) || !generated);
    CHECK(!g.serves(100, 7, 5) || !generated);
    const GlobalPhotons::DeviceSource a = g.source_on(fake_device(0)), b = g.source_on(fake_device(1));
    CHECK(a.photons == on_a && b.photons == on_b);
    CHECK(!a || a.n == n);
    CHECK(!b || b.n == n);
    CHECK(!g.source_on(nullptr) && !g.source_on(fake_device(2)));
    CHECK(generated || (g.skip().empty() && g.host_raw().empty() && !g.device() && !g.host_copy_missing()));
}

// to_host of rt_photons.cpp: the map comes to the host from the device it lies on, once
static void fetch(GlobalPhotons &g, const std::vector<rt_photon> &device_memory)
{
    if (!g.host_copy_missing()) return;
    const GlobalPhotons::DeviceSource src = g.source_on(g.device());
    CHECK(src && src.photons == device_memory.data());
    g.set_host_copy(std::vector<rt_photon>(src.photons, src.photons + src.n + 1));
}
// leaving_device of rt_photons.cpp
static void leaving_device(GlobalPhotons &g, DeviceState *D, const std::vector<rt_photon> &device_memory)
{
    if (!g.source_on(D)) return;
    fetch(g, device_memory);
    g.leave_device(D);
}

int main()
{
    DeviceState *A = fake_device(0), *B = fake_device(1);
    std::vector<rt_photon> balanced;                        // SceneData::photons
    std::vector<rt_photon> callers(8), mem_a(6), mem_b(5);  // a caller's map of 7; the pass buffers of A (5 photons) and B (4)
    for (size_t i = 0; i < callers.size(); i++) callers[i].position[0] = 100.0f + (float)i;
    for (size_t i = 0; i < mem_a.size(); i++) mem_a[i].position[0] = 10.0f + (float)i;
    for (size_t i = 0; i < mem_b.size(); i++) mem_b[i].position[0] = 20.0f + (float)i;
    GlobalPhotons g;

    expect(g, 0, false, false, false, nullptr, nullptr);                                    // none
    CHECK(!g.drop_generated(balanced));
    g.leave_device(A);
    expect(g, 0, false, false, false, nullptr, nullptr);

    g.set_callers(balanced, callers.data(), 7);                                             // -> the caller's
    expect(g, 7, false, true, true, nullptr, nullptr);
    CHECK(balanced.size() == 8 && balanced[7].position[0] == 107.0f);

    g.adopt_generated(balanced, A, mem_a.data(), 5, {100, 8, 5}, {4, 5}, {});               // -> generated, on A only
    expect(g, 5, true, true, false, mem_a.data(), nullptr);
    CHECK(balanced.empty() && g.host_copy_missing() && g.device() == A && g.skip().size() == 2);

    leaving_device(g, B, mem_b);                                                            // a pass on another device: nothing moves
    expect(g, 5, true, true, false, mem_a.data(), nullptr);
    CHECK(g.host_copy_missing());

    leaving_device(g, A, mem_a);                                                            // a pass on A: host copy appears, residence gone
    expect(g, 5, true, true, false, nullptr, nullptr);
    CHECK(!g.host_copy_missing() && !g.device() && g.host_raw().size() == 6 && g.host_raw()[5].position[0] == 15.0f && g.skip().size() == 2);
    mem_a.assign(3, rt_photon{});                                                           // A's buffer now holds something else, smaller
    leaving_device(g, A, mem_a);                                                            // ... and another pass there changes nothing
    expect(g, 5, true, true, false, nullptr, nullptr);
    balanced.assign(6, rt_photon{});                                                        // rt_scene_get_photons balanced it

    g.adopt_generated(balanced, B, mem_b.data(), 4, {100, 8, 6}, {}, std::vector<rt_photon>(mem_b));    // -> adopted on B, with a host copy (.dat dump)
    expect(g, 4, true, false, true, nullptr, mem_b.data());
    CHECK(balanced.empty() && !g.host_copy_missing() && g.device() == B && g.skip().empty());
    leaving_device(g, B, mem_b);                                                            // both -> host only
    expect(g, 4, true, false, true, nullptr, nullptr);
    CHECK(g.host_raw().size() == 5);

    balanced.assign(5, rt_photon{});
    CHECK(g.drop_generated(balanced));                                                      // -> dropped by a geometry change
    expect(g, 0, false, false, false, nullptr, nullptr);
    CHECK(balanced.empty());

    g.set_callers(balanced, callers.data(), 7);                                             // the caller's map survives one
    CHECK(!g.drop_generated(balanced));
    expect(g, 7, false, true, true, nullptr, nullptr);
    CHECK(balanced.size() == 8);

    g.adopt_generated(balanced, A, mem_b.data(), 4, {100, 8, 5}, {3}, {});                  // generated (device only) replaced by set_photons
    expect(g, 4, true, true, false, mem_b.data(), nullptr);
    g.set_callers(balanced, callers.data(), 3);
    expect(g, 3, false, true, true, nullptr, nullptr);
    CHECK(balanced.size() == 4);
    g.adopt_generated(balanced, A, mem_b.data(), 4, {100, 8, 5}, {3}, std::vector<rt_photon>(mem_b));   // ... and one with a host copy by "no map"
    g.set_callers(balanced, nullptr, 0);
    expect(g, 0, false, false, false, nullptr, nullptr);
    CHECK(balanced.empty());

    printf("ok %d steps\n", g_step);
    return 0;
}
