// shim_driver_util.h -- test infrastructure: what more than one tests/shim_*_driver.cpp defines the same way.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>

#include "../raytracing_folder_amd/csrc/host/rt_shim.h"

// BeginRender() + WaitRender(); a failure is said on stderr
static inline bool render(rt::Renderer &r)
{
    if (!r.BeginRender()) { fprintf(stderr, "BeginRender failed: %s\n", r.LastError().c_str()); return false; }
    if (!r.WaitRender()) { fprintf(stderr, "render failed: %s\n", r.LastError().c_str()); return false; }
    return true;
}

// n raw bytes to the file `name`
static inline bool dump(const std::string &name, const uint8_t *p, size_t n)
{
    FILE *f = fopen(name.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(p, 1, n, f) == n;
    return fclose(f) == 0 && ok;
}
