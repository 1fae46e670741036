// The host mirror of the device tree build as a program of its own (TEST INFRASTRUCTURE): csrc/rt_lbvh.h compiled alone -- no
// HIP, no library -- so that another compiler, and a host-only build under -fsanitize=address,undefined, run the very functions
// the kernels are made of.  tests/test_lbvh_host.py builds and runs it.
//   lbvh_mirror_driver <mesh file> <out file>
// mesh file: uint32 nv, nf; nv x 3 float32; nf x 3 uint32.  stdout: n_nodes root_ref stack_need.  out file: the node records, then slot_face.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../raytracing_folder_amd/csrc/rt_lbvh.h"

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s mesh.bin out.bin\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 2; }
    uint32_t head[2];
    if (fread(head, 4, 2, in) != 2 || head[0] == 0 || head[1] == 0) { fprintf(stderr, "bad header\n"); return 2; }
    std::vector<float> v(3 * (size_t)head[0]);
    std::vector<uint32_t> f(3 * (size_t)head[1]);
    if (fread(v.data(), 4, v.size(), in) != v.size() || fread(f.data(), 4, f.size(), in) != f.size()) { fprintf(stderr, "short file\n"); return 2; }
    fclose(in);
    for (const uint32_t i : f) if (i >= head[0]) { fprintf(stderr, "face index out of range\n"); return 2; }
    std::vector<LbvhRecord> nodes;
    std::vector<uint32_t> slot_face, level_off;
    uint32_t root_ref = 0;
    int need = 0;
    lbvh_build_host(v.data(), f.data(), head[1], nodes, slot_face, root_ref, need, &level_off);
    if (level_off.back() != nodes.size()) { fprintf(stderr, "level_off ends at %u of %zu records\n", level_off.back(), nodes.size()); return 1; }
    FILE *out = fopen(argv[2], "wb");
    if (!out) { perror(argv[2]); return 2; }
    if (!nodes.empty()) fwrite(nodes.data(), sizeof(LbvhRecord), nodes.size(), out);
    fwrite(slot_face.data(), 4, slot_face.size(), out);
    fclose(out);
    printf("%zu %u %d\n", nodes.size(), root_ref, need);
    return 0;
}
