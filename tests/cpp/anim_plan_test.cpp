// The rules and layouts of the animation set-up (csrc/fovpt_animplan.h) as a stand-alone host program, for
// tests/test_anim_plan_cpu.py: reads commands from standard input and prints what the header answers.  Built with the address and
// undefined-behaviour sanitizers; no HIP, nothing preloaded.
//
// Every array comes as its REAL length (-1: a null pointer) and that many values, apart from the count the description states,
// and is allocated at exactly that length: a read beyond what the earlier rules admitted is the sanitizer's to report.  Floats
// travel as their 32 bits, doubles as their 64 bits, both as unsigned integers.
//
//   SCENE := NMESH (nv skin_joints pal_first morph_targets w_first morph_entries) x NMESH
//   skins SCENE NUM REAL (mesh nv nj reserved JOINTS WEIGHTS) x REAL
//   morphs | morph_counts SCENE NUM REAL (mesh nv nt reserved TREAL (count reserved INDEX DELTA) x TREAL) x REAL
//   rig SCENE r0 r1 r2 num_nodes num_bindings num_clips  NREAL (parent 10 floats) x NREAL
//       BREAL (mesh node nj reserved JOINT_NODES INVERSE_BIND) x BREAL
//       CREAL (num_channels reserved HREAL (target path interpolation num_keys TIMES VALUES) x HREAL) x CREAL
//   transform MESH A 12 floats | palette WHO MESH NJ S B MATRICES | weights MESH NT WEIGHTS DS A
//   list WHO NMESH NUM meshes (the meshes a list names, in its order) | norm 4 floats (rig_norm_ok)
//
// Answer: "code C", "text ...", for an accepted plan one line per table ("name n values"), then "end".
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "fovpt_animplan.h"

template <class T> struct Array {
    std::unique_ptr<T[]> p;
    long n = -1;
    const T* get() const { return n < 0 ? nullptr : p.get(); }
};

template <class T> static Array<T> read_array(std::istream& in)
{
    Array<T> a;
    in >> a.n;
    if (a.n < 0) return a;
    a.p.reset(new T[(size_t)a.n]);
    for (long i = 0; i < a.n; i++) {
        unsigned long long v = 0;
        in >> v;
        if (sizeof(T) == 8) { const uint64_t b = v; memcpy(&a.p[i], &b, 8); }
        else if (sizeof(T) == 4) { const uint32_t b = (uint32_t)v; memcpy(&a.p[i], &b, 4); }
        else { const uint16_t b = (uint16_t)v; memcpy(&a.p[i], &b, 2); }
    }
    return a;
}

static float read_float(std::istream& in) { uint32_t b = 0; in >> b; float f; memcpy(&f, &b, 4); return f; }
static double read_double(std::istream& in) { unsigned long long b = 0; in >> b; const uint64_t u = b; double d; memcpy(&d, &u, 8); return d; }
static unsigned bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }
static unsigned long long bits(double d) { uint64_t b; memcpy(&b, &d, 8); return b; }

static AnimScene read_scene(std::istream& in)
{
    AnimScene sc;
    size_t n = 0;
    in >> n;
    sc.mesh.resize(n);
    for (AnimMesh& M : sc.mesh) in >> M.nv >> M.skin_joints >> M.pal_first >> M.morph_targets >> M.w_first >> M.morph_entries;
    return sc;
}

static void verdict(const AnimVerdict& V) { printf("code %d\ntext %s\n", V.code, V.text.c_str()); }
template <class T> static void table(const char* name, const std::vector<T>& v)
{
    printf("%s %zu", name, v.size());
    for (const T& x : v) printf(" %lld", (long long)x);
    printf("\n");
}
static void table(const char* name, const std::vector<float>& v)
{
    printf("%s %zu", name, v.size());
    for (float x : v) printf(" %u", bits(x));
    printf("\n");
}
static void table(const char* name, const std::vector<double>& v)
{
    printf("%s %zu", name, v.size());
    for (double x : v) printf(" %llu", bits(x));
    printf("\n");
}

static void do_skins(std::istream& in)
{
    const AnimScene sc = read_scene(in);
    int num = 0;
    long real = 0;
    in >> num >> real;
    std::unique_ptr<fovpt_mesh_skin[]> skins(real < 0 ? nullptr : new fovpt_mesh_skin[(size_t)real]);
    std::vector<Array<uint16_t>> joints;
    std::vector<Array<float>> weights;
    for (long k = 0; k < real; k++) {
        fovpt_mesh_skin& K = skins[k];
        in >> K.mesh >> K.num_vertices >> K.num_joints >> K._reserved;
        joints.push_back(read_array<uint16_t>(in));
        weights.push_back(read_array<float>(in));
        K.joints = joints.back().get(); K.weights = weights.back().get();
    }
    SkinPlan P;
    plan_skins(sc, "fovpt_set_skins", skins.get(), num, P);
    verdict(P);
    if (!P.code) {
        table("S", P.S); table("num_joints", P.num_joints); table("first", P.first); table("pal_first", P.pal_first);
        printf("totals 2 %zu %zu\nbytes 3 %zu %zu %zu\n", P.verts, P.joints, P.joints_bytes, P.weights_bytes, P.pal_bytes);
    }
    printf("end\n");
}

static void do_morphs(std::istream& in, bool counts_only)
{
    const AnimScene sc = read_scene(in);
    int num = 0;
    long real = 0;
    in >> num >> real;
    std::unique_ptr<fovpt_mesh_morph[]> morphs(real < 0 ? nullptr : new fovpt_mesh_morph[(size_t)real]);
    std::vector<std::unique_ptr<fovpt_morph_target[]>> targets;
    std::vector<Array<uint32_t>> index;
    std::vector<Array<float>> delta;
    for (long k = 0; k < real; k++) {
        fovpt_mesh_morph& K = morphs[k];
        long treal = 0;
        in >> K.mesh >> K.num_vertices >> K.num_targets >> K._reserved >> treal;
        targets.emplace_back(treal < 0 ? nullptr : new fovpt_morph_target[(size_t)treal]);
        K.targets = targets.back().get();
        for (long t = 0; t < treal; t++) {
            fovpt_morph_target& T = targets.back()[t];
            in >> T.count >> T._reserved;
            index.push_back(read_array<uint32_t>(in));
            delta.push_back(read_array<float>(in));
            T.index = index.back().get(); T.delta = delta.back().get();
        }
    }
    MorphPlan P;
    if (counts_only) plan_morph_counts(sc, "fovpt_set_morphs", morphs.get(), num, P);
    else plan_morphs(sc, "fovpt_set_morphs", morphs.get(), num, P);
    verdict(P);
    if (!P.code) {
        table("entries", P.entries); table("num_targets", P.num_targets); table("num_entries", P.num_entries);
        printf("totals 3 %zu %zu %zu\n", P.offs, P.ents, P.targets);
        for (size_t k = 0; k < P.listed.size(); k++) {
            const MorphPlan::Listed& D = P.listed[k];
            table(("off" + std::to_string(k)).c_str(), D.off);
            printf("ent%zu %zu", k, 4 * D.ent.size());
            for (const MorphEntry& e : D.ent) printf(" %u %u %u %u", bits(e.dx), bits(e.dy), bits(e.dz), e.target);
            printf("\n");
            table(("D" + std::to_string(k)).c_str(), D.D);
        }
        if (!counts_only) {
            table("off_first", P.off_first); table("ent_first", P.ent_first); table("w_first", P.w_first);
            printf("bytes 3 %zu %zu %zu\n", P.off_bytes, P.ent_bytes, P.w_bytes);
        }
    }
    printf("end\n");
}

static void do_rig(std::istream& in)
{
    const AnimScene sc = read_scene(in);
    fovpt_rig_desc rig = {};
    in >> rig._reserved0 >> rig._reserved1 >> rig._reserved2 >> rig.num_nodes >> rig.num_bindings >> rig.num_clips;
    long nreal = 0, breal = 0, creal = 0;
    in >> nreal;
    std::unique_ptr<fovpt_rig_node[]> nodes(nreal < 0 ? nullptr : new fovpt_rig_node[(size_t)nreal]);
    for (long i = 0; i < nreal; i++) {
        fovpt_rig_node& N = nodes[i];
        in >> N.parent;
        for (float& x : N.translation) x = read_float(in);
        for (float& x : N.rotation) x = read_float(in);
        for (float& x : N.scale) x = read_float(in);
    }
    in >> breal;
    std::unique_ptr<fovpt_rig_binding[]> bindings(breal < 0 ? nullptr : new fovpt_rig_binding[(size_t)breal]);
    std::vector<Array<uint16_t>> joint_nodes;
    std::vector<Array<float>> floats;
    for (long k = 0; k < breal; k++) {
        fovpt_rig_binding& B = bindings[k];
        in >> B.mesh >> B.node >> B.num_joints >> B._reserved;
        joint_nodes.push_back(read_array<uint16_t>(in));
        floats.push_back(read_array<float>(in));
        B.joint_nodes = joint_nodes.back().get(); B.inverse_bind = floats.back().get();
    }
    in >> creal;
    std::unique_ptr<fovpt_rig_clip[]> clips(creal < 0 ? nullptr : new fovpt_rig_clip[(size_t)creal]);
    std::vector<std::unique_ptr<fovpt_rig_channel[]>> channels;
    for (long k = 0; k < creal; k++) {
        fovpt_rig_clip& K = clips[k];
        long hreal = 0;
        in >> K.num_channels >> K._reserved >> hreal;
        channels.emplace_back(hreal < 0 ? nullptr : new fovpt_rig_channel[(size_t)hreal]);
        K.channels = channels.back().get();
        for (long h = 0; h < hreal; h++) {
            fovpt_rig_channel& H = channels.back()[h];
            in >> H.target >> H.path >> H.interpolation >> H.num_keys;
            floats.push_back(read_array<float>(in));
            H.times = floats.back().get();
            floats.push_back(read_array<float>(in));
            H.values = floats.back().get();
        }
    }
    rig.nodes = nodes.get(); rig.bindings = bindings.get(); rig.clips = clips.get();
    RigPlan P;
    plan_rig(sc, "fovpt_set_rig", &rig, P);
    verdict(P);
    if (!P.code) {
        table("parent", P.parent); table("level", P.level); table("rest", P.rest);
        printf("bound %zu", 5 * P.bound.size());
        for (const RigBound& b : P.bound) printf(" %d %u %d %d %d", b.mesh, b.rigid, (int)b.skinned, (int)b.morphed, (int)b.is_rigid);
        printf("\n");
        table("pal_node", P.pal_node); table("pal_dst", P.pal_dst); table("inv_bind", P.inv_bind); table("rigid_node", P.rigid_node);
        printf("wjobs %zu", 2 * P.wjobs.size());
        for (const RigWeights& w : P.wjobs) printf(" %u %u", w.w_first, w.num_targets);
        printf("\n");
        table("node_chan", P.node_chan); table("w_chan", P.w_chan);
        printf("chan %zu", 4 * P.chan.size());
        for (const RigChannel& c : P.chan) printf(" %u %u %u %u", c.t_first, c.v_first, c.num_keys, c.interp);
        printf("\n");
        table("times", P.times); table("values", P.values);
        printf("at %d", (int)RIG_SECTIONS);
        for (size_t a : P.at) printf(" %zu", a);
        printf("\nscalars 5 %u %u %u %u %zu\n", P.num_nodes, P.num_clips, P.num_levels, P.threads, P.outs);
        printf("blob %zu", P.blob.size());
        for (char b : P.blob) printf(" %u", (unsigned)(unsigned char)b);
        printf("\n");
    }
    printf("end\n");
}

int main()
{
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "skins") do_skins(std::cin);
        else if (cmd == "morphs") do_morphs(std::cin, false);
        else if (cmd == "morph_counts") do_morphs(std::cin, true);
        else if (cmd == "rig") do_rig(std::cin);
        else if (cmd == "transform") {
            int mesh = 0;
            std::cin >> mesh;
            const double A = read_double(std::cin);
            float m[12];
            for (float& x : m) x = read_float(std::cin);
            AnimVerdict V;
            anim_check_transform(V, "fovpt_update_transforms", mesh, m, A);
            verdict(V);
            printf("end\n");
        } else if (cmd == "palette") {
            int mesh = 0;
            uint32_t nj = 0;
            std::string who;
            std::cin >> who >> mesh >> nj;
            const double S = read_double(std::cin), B = read_double(std::cin);
            const Array<float> m = read_array<float>(std::cin);
            AnimVerdict V;
            anim_check_palette(V, who.c_str(), mesh, m.get(), nj, S, B);
            verdict(V);
            printf("end\n");
        } else if (cmd == "weights") {
            int mesh = 0;
            uint32_t nt = 0;
            std::cin >> mesh >> nt;
            const Array<float> w = read_array<float>(std::cin);
            const Array<double> D = read_array<double>(std::cin);
            const double A = read_double(std::cin);
            double B = 0.0;
            AnimVerdict V;
            anim_check_weights(V, "fovpt_update_morphed", mesh, w.get(), nt, D.get(), A, &B);
            verdict(V);
            printf("B 1 %llu\nend\n", bits(B));
        } else if (cmd == "list") {
            std::string who;
            size_t nmesh = 0, num = 0;
            std::cin >> who >> nmesh >> num;
            std::vector<char> seen(nmesh, 0);
            AnimVerdict V;
            for (size_t k = 0; k < num; k++) {
                int m = 0;
                std::cin >> m;
                if (!V.code) anim_list_mesh(V, seen, who.c_str(), m);
            }
            verdict(V);
            printf("end\n");
        } else if (cmd == "norm") {
            float q[4];
            for (float& x : q) x = read_float(std::cin);
            printf("code %d\ntext \nend\n", rig_norm_ok(q) ? 0 : FOVPT_E_INVALID);
        } else {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
        if (!std::cin) { fprintf(stderr, "truncated input in %s\n", cmd.c_str()); return 2; }
    }
    return 0;
}
