// host_model.cpp -- models: validation and upload, culling bounds and chunk tables, the palette ring, skeleton and pose.
#include "host.h"

// k_pose.hip.  Weak: the host-only builds of this file (tests/cpp, over the HIP stub runtime) link no kernels and never
// form a pose; libmtr.so links k_pose.o.
void mtr_launch_pose(const PoseParams& p, uint32_t ninst, hipStream_t s) __attribute__((weak));

namespace mtr_host {

namespace {

// src/shaders/debug_ids.wgsl:23-44
const uint8_t kDebugPalette[20][3] = {
    {215, 62, 103}, {95, 190, 80},  {133, 95, 213},  {180, 184, 53},  {213, 87, 180}, {72, 138, 55},  {145, 79, 158},
    {91, 196, 153}, {206, 78, 55},  {74, 174, 209},  {225, 133, 58},  {92, 122, 198}, {207, 162, 81}, {188, 144, 216},
    {152, 173, 92}, {161, 71, 103}, {53, 133, 98},   {225, 131, 152}, {111, 111, 40}, {162, 99, 55},
};

// bytes a float-class element reads, 0 = not in the reference's table (src/rshader2.rs:516-564)
uint32_t elem_bytes(uint8_t fmt, uint8_t cnt) {
    switch (fmt) {
    case MTR_IEF_U8N: return cnt == 1 ? 2 : cnt == 4 ? 4 : 0;
    case MTR_IEF_S8N: return cnt == 1 ? 2 : (cnt == 3 || cnt == 4) ? 4 : 0;
    case MTR_IEF_S16N: return cnt == 1 ? 4 : cnt == 3 ? 8 : 0;
    case MTR_IEF_F16: return cnt == 2 ? 4 : 0;
    case MTR_IEF_F32: return cnt == 3 ? 12 : 0;
    case MTR_IEF_U8NL: return cnt == 3 ? 4 : 0;
    case MTR_IEF_SCMP3N: return 4;  // only reached with MTR_ELEM_DECODE_SCMP3N
    default: return 0;
    }
}

// ---- host mirror of the position decode (csrc/geom_vertex.h: decode_regs, decode_elem), for the culling bounds ----
float h_half(uint16_t h) {
    const uint32_t sign = (uint32_t)(h >> 15) << 31, ex = (h >> 10) & 0x1f, man = h & 0x3ff;
    uint32_t bits;
    if (ex == 0) {
        if (man == 0) bits = sign;
        else {  // subnormal: man * 2^-24
            float f = (float)man * 5.9604644775390625e-08f;
            memcpy(&bits, &f, 4);
            bits |= sign;
        }
    } else if (ex == 31) bits = sign | 0x7f800000u | (man << 13);
    else bits = sign | ((ex + 112) << 23) | (man << 13);
    float f;
    memcpy(&f, &bits, 4);
    return f;
}
float h_snorm16(uint16_t v) { float f = (float)(int16_t)v / 32767.0f; return f < -1.0f ? -1.0f : f; }
float h_snorm8(uint8_t v) { float f = (float)(int8_t)v / 127.0f; return f < -1.0f ? -1.0f : f; }
float h_unorm8(uint8_t v) { return (float)v / 255.0f; }
uint16_t h_ld16(const uint8_t* p) { return (uint16_t)(p[0] | (p[1] << 8)); }

void decode_pos_host(uint32_t fmt, uint32_t cnt, const uint8_t* p, float (&o)[3]) {
    o[0] = o[1] = o[2] = 0.0f;
    switch (fmt) {
    case MTR_IEF_U8N: case MTR_IEF_U8NL:
        o[0] = h_unorm8(p[0]); o[1] = h_unorm8(p[1]);
        if (!(fmt == MTR_IEF_U8N && cnt == 1)) o[2] = h_unorm8(p[2]);
        break;
    case MTR_IEF_S8N:
        o[0] = h_snorm8(p[0]); o[1] = h_snorm8(p[1]);
        if (cnt != 1) o[2] = h_snorm8(p[2]);
        break;
    case MTR_IEF_S16N:
        o[0] = h_snorm16(h_ld16(p)); o[1] = h_snorm16(h_ld16(p + 2));
        if (cnt == 3) o[2] = h_snorm16(h_ld16(p + 4));
        break;
    case MTR_IEF_F16:
        o[0] = h_half(h_ld16(p)); o[1] = h_half(h_ld16(p + 2));
        break;
    case MTR_IEF_F32:
        memcpy(&o[0], p, 4); memcpy(&o[1], p + 4, 4); memcpy(&o[2], p + 8, 4);
        break;
    case MTR_IEF_SCMP3N: {
        uint32_t w;
        memcpy(&w, p, 4);
        for (int k = 0; k < 3; k++) {
            const float f = (float)((int32_t)((w >> (10 * k)) << 22) >> 22) / 511.0f;
            o[k] = f < -1.0f ? -1.0f : f;
        }
        break;
    }
    default: break;
    }
}

struct BoxAcc {
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    bool any = false, bad = false;
    void add(const float (&p)[3]) {
        for (int k = 0; k < 3; k++) {
            if (!(std::fabs(p[k]) < 3.0e38f)) bad = true;  // NaN / inf position: the box cannot hold it
            lo[k] = std::min(lo[k], (double)p[k]); hi[k] = std::max(hi[k], (double)p[k]);
        }
        any = true;
    }
    void merge(const BoxAcc& o) {
        if (!o.any) return;
        for (int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], o.lo[k]); hi[k] = std::max(hi[k], o.hi[k]); }
        any = true; bad = bad || o.bad;
    }
    BoneBox box(uint32_t joint) const {
        BoneBox b{};
        float* c = &b.cx; float* e = &b.ex;
        for (int k = 0; k < 3; k++) {
            const float cf = (float)((lo[k] + hi[k]) * 0.5);
            const double ext = std::max(hi[k] - (double)cf, (double)cf - lo[k]);
            c[k] = cf;
            e[k] = std::nextafter((float)ext, INFINITY);  // rounded up
            if (bad) e[k] = INFINITY;                      // the test sees a non-finite interval and keeps the geometry
        }
        b.joint = joint;
        return b;
    }
};

// Chunk and whole-model bounds of a new model (vertex bytes still on the host).  boxes: the d_boxes image.
void build_bounds(mtr_model* m, const uint8_t* vbuf, std::vector<BoneBox>& boxes, std::vector<BoneBox>& inst_boxes) {
    const size_t nprims = m->prims.size();
    m->prim_chunk_base.assign(nprims + 1, 0);
    for (size_t p = 0; p < nprims; p++)
        m->prim_chunk_base[p + 1] = m->prim_chunk_base[p] + (m->prims[p].index_num + MTR_CHUNK_NEW - 1) / MTR_CHUNK_NEW;
    const size_t nstatic = m->prim_chunk_base[nprims];
    m->cb_first.assign(nstatic, 0); m->cb_count.assign(nstatic, 0); m->cb_flags.assign(nstatic, 0);
    BoxAcc all_unskinned, rigid_part;   // every vertex / the vertices of primitives that cannot be skinned
    std::vector<BoxAcc> joint_acc(256);
    bool weights_ok = true;
    struct JA { uint32_t joint; BoxAcc acc; };
    std::vector<JA> ja;
    for (size_t p = 0; p < nprims; p++) {
        const DPrim& pr = m->prims[p];
        const uint8_t* vb = vbuf + pr.vertex_base;
        for (uint32_t start = 0, k = 0; start < pr.index_num; start += MTR_CHUNK_NEW, k++) {
            const size_t sc = m->prim_chunk_base[p] + k;
            BoxAcc whole;
            ja.clear();
            uint32_t flags = 0;
            const uint32_t lo = start >= 2 ? start - 2 : 0, hi = std::min(pr.index_num, start + MTR_CHUNK_NEW);
            for (uint32_t q = lo; q < hi; q++) {
                const uint32_t idx = m->indices[pr.index_ofs + q];
                if (pr.topology == 4 && idx == 0xFFFFu) continue;
                const uint32_t vid = idx + pr.index_base;
                if (vid >= pr.vertex_num) continue;
                const uint8_t* vp = vb + (size_t)vid * pr.stride;
                float pos[3];
                decode_pos_host(pr.pos_fmt, pr.pos_cnt, vp + pr.pos_off, pos);
                whole.add(pos);
                if (!pr.skinnable) continue;
                const uint8_t* jp = vp + pr.joint_off; const uint8_t* wp = vp + pr.weight_off;
                if ((uint32_t)wp[0] + wp[1] + wp[2] + wp[3] != 255u) { flags |= 1u; weights_ok = false; }
                for (int t = 0; t < 4; t++) {
                    if (wp[t] == 0) continue;  // contributes exactly nothing to the blend
                    joint_acc[jp[t]].add(pos);
                    size_t e = 0;
                    while (e < ja.size() && ja[e].joint != jp[t]) e++;
                    if (e == ja.size()) ja.push_back({jp[t], BoxAcc()});
                    ja[e].acc.add(pos);
                }
            }
            all_unskinned.merge(whole);
            if (!pr.skinnable) rigid_part.merge(whole);
            if (!whole.any) continue;  // no vertex: nothing to bound (the chunk is kept, it has no triangle anyway)
            if (ja.size() > MTR_CHUNK_MAX_BOXES) { flags |= 1u; ja.clear(); }
            m->cb_first[sc] = (uint32_t)boxes.size();
            m->cb_count[sc] = 1u + (uint32_t)ja.size();
            m->cb_flags[sc] = flags;
            boxes.push_back(whole.box(MTR_BOX_UNSKINNED));
            for (const JA& e : ja) boxes.push_back(e.acc.box(e.joint));
        }
    }
    inst_boxes.clear();
    if (all_unskinned.any) inst_boxes.push_back(all_unskinned.box(MTR_BOX_UNSKINNED));
    m->n_inst_unskinned = (uint32_t)inst_boxes.size();
    if (rigid_part.any) inst_boxes.push_back(rigid_part.box(MTR_BOX_UNSKINNED));
    for (uint32_t j = 0; j < 256; j++)
        if (joint_acc[j].any) inst_boxes.push_back(joint_acc[j].box(j));
    m->n_inst_skinned = (uint32_t)inst_boxes.size() - m->n_inst_unskinned;
    m->inst_skinned_boundable = weights_ok;
}

void rebuild_chunks(const mtr_model* m, ChunkTable* t) {
    t->chunks.clear();
    t->ntris_visible = 0;
    for (size_t p = 0; p < m->prims.size(); p++) {
        const DPrim& pr = m->prims[p];
        if (pr.parts_no >= m->parts_disp.size() || !m->parts_disp[pr.parts_no]) continue;  // src/model.rs:318-320
        for (uint32_t start = 0; start < pr.index_num; start += MTR_CHUNK_NEW) {
            DChunk c;
            c.prim = (uint32_t)p;
            c.start = start;
            c.q_before = start >= 3 ? m->run[pr.index_ofs + start - 3] : 0;
            // the run must not reach back before this primitive's first index
            if (start >= 3 && c.q_before > start - 2) c.q_before = start - 2;
            uint32_t nt = 0, end = std::min(pr.index_num, start + MTR_CHUNK_NEW);
            for (uint32_t q = start; q < end; q++) {
                if (pr.topology == 4) {
                    uint32_t r = std::min(m->run[pr.index_ofs + q], q + 1);
                    nt += r >= 3;
                } else {
                    nt += (q % 3 == 2);
                }
            }
            c.ntris = nt;
            const size_t sc = m->prim_chunk_base[p] + start / MTR_CHUNK_NEW;
            c.b_first = m->cb_first[sc]; c.b_count = m->cb_count[sc]; c.b_flags = m->cb_flags[sc] | (pr.skinnable ? 2u : 0u); c.pad = 0;
            t->ntris_visible += nt;
            t->chunks.push_back(c);
        }
    }
}

}  // namespace

// The k_pose path table of a skeleton: paths[j] = offset | length << 16 of joint j's path in `bytes`, the joints from its
// root down to j (a root's path is itself).  false: a parent out of range or a cycle.
bool pose_paths(const uint8_t* parents, size_t n, std::vector<uint32_t>& paths, std::vector<uint8_t>& bytes) {
    std::vector<uint8_t> state(n, 0);  // 0 new, 1 on the walk, 2 checked
    for (size_t j0 = 0; j0 < n; j0++) {
        std::vector<size_t> walk;
        size_t j = j0;
        while (state[j] != 2) {
            if (state[j] == 1) return false;  // its own ancestor
            state[j] = 1;
            walk.push_back(j);
            const uint32_t p = parents[j];
            if (p == 255 || p == j) break;
            if (p >= n) return false;
            j = p;
        }
        for (size_t c : walk) state[c] = 2;
    }
    paths.assign(n, 0);
    bytes.clear();
    std::vector<uint8_t> up;
    for (size_t j = 0; j < n; j++) {
        up.clear();
        for (size_t k = j;; k = parents[k]) {
            up.push_back((uint8_t)k);
            if (parents[k] == 255 || parents[k] == k) break;
        }
        paths[j] = (uint32_t)bytes.size() | ((uint32_t)up.size() << 16);
        bytes.insert(bytes.end(), up.rbegin(), up.rend());
    }
    bytes.resize((bytes.size() + 3) & ~size_t(3), 0);
    return true;
}

// The model's chunk table for its current parts_disp, built and uploaded on first use.  submit_mu held.
int32_t current_table(mtr_model* m, std::shared_ptr<const ChunkTable>* out) {
    mtr_device* d = m->dev;
    if (m->chunks_dirty || !m->table) {
        auto t = std::make_shared<ChunkTable>();
        t->hip_dev = d->hip_dev;
        rebuild_chunks(m, t.get());
        int32_t rc = dev_alloc(d, &t->d_chunks, t->chunks.size());
        if (rc) return rc;
        if (!t->chunks.empty()) HIPCHK(d, hipMemcpy(t->d_chunks, t->chunks.data(), t->chunks.size() * sizeof(DChunk), hipMemcpyHostToDevice));
        m->table = std::move(t);
        m->chunks_dirty = false;
    }
    *out = m->table;
    return MTR_OK;
}

// The next buffer of the model's palette ring for an n-matrix palette, made current (see mtr_model::PalBuf).  submit_mu held.
int32_t next_palette_buffer(mtr_model* m, size_t n, mtr_model::PalBuf** out) {
    mtr_device* d = m->dev;
    int32_t rc = MTR_OK;
    if (m->pal_ring.size() < (size_t)d->max_inflight + 1)  // first use (the bound is fixed at device creation)
        m->pal_ring.resize((size_t)d->max_inflight + 1);
    size_t slot = m->pal_next++ % m->pal_ring.size();
    for (size_t tries = 0; m->pal_ring[slot].pinned && tries < m->pal_ring.size(); tries++) slot = m->pal_next++ % m->pal_ring.size();
    if (m->pal_ring[slot].pinned) {
        // every buffer is held by a live frame that may still (re-)run: the host keeps more un-waited frames alive than
        // the ring has buffers.  The ring grows by one (indices held by recorded draws stay valid).
        if (m->pal_ring.size() >= 4096) return fail(d, MTR_E_NOMEM, "more than 4096 live frames hold a palette of this model");
        m->pal_ring.emplace_back();
        slot = m->pal_ring.size() - 1;
    }
    mtr_model::PalBuf& pb = m->pal_ring[slot];
    // the last frame that read this buffer: finished for sure once max_inflight later frames have been submitted
    if (pb.used && d->frames_submitted < pb.last_frame + 1 + d->max_inflight && d->inflight[pb.last_frame % d->max_inflight])
        HIPCHK(d, hipEventSynchronize(d->inflight[pb.last_frame % d->max_inflight]));
    if (pb.cap < n) {  // grow: nothing in flight may still read the old buffer
        if ((rc = drain_all(d))) return rc;
        if (pb.d) (void)hipFree(pb.d);
        pb.d = nullptr; pb.cap = 0;
        if ((rc = dev_alloc(d, &pb.d, std::max<size_t>(n, 64) * 16))) return rc;
        pb.cap = (uint32_t)std::max<size_t>(n, 64);
    }
    if (!pb.ready) HIPCHK(d, hipEventCreateWithFlags(&pb.ready, hipEventDisableTiming));
    m->npal = (uint32_t)n;
    m->d_palette = pb.d;
    m->pal_ready = pb.ready;
    m->pal_slot = (int)slot;
    *out = &pb;
    return MTR_OK;
}

}  // namespace mtr_host

using namespace mtr_host;

extern "C" {

// ---------------------------------------------------------------------------------------------
// Model::new
// ---------------------------------------------------------------------------------------------
int32_t mtr_model_create(mtr_device* d, const void* vertex_buf, size_t vertex_len, const uint16_t* index_buf,
                         size_t index_num, const mtr_primitive* prims, size_t nprims, const mtr_layout* layouts,
                         const int32_t* prim_to_texture, mtr_texture* const* textures, size_t ntextures,
                         const uint32_t* prim_debug_id, mtr_model** out) {
    if (!d || !out) return MTR_E_INVALID;
    *out = nullptr;
    if (!vertex_buf || !index_buf || !prims || !layouts || nprims == 0 || nprims > 0xFFFF)
        return fail(d, MTR_E_INVALID, "null or empty model input");
    if (index_num > 0x7FFFFFFFu || vertex_len > 0xFFFFFFFFu) return fail(d, MTR_E_INVALID, "model too large");
    auto m = std::make_unique<mtr_model>();
    m->dev = d;
    m->vertex_len = vertex_len;
    m->prims.resize(nprims);
    m->prim_to_texture.assign(nprims, -1);
    m->debug_rgba8.resize(nprims);
    for (size_t t = 0; t < ntextures; t++) {
        if (!textures || !textures[t] || textures[t]->dev != d) return fail(d, MTR_E_INVALID, "bad texture handle");
        m->textures.push_back(textures[t]);
    }
    for (size_t p = 0; p < nprims; p++) {
        const uint32_t* w = prims[p].w;  // bit-fields: src/rmodel.rs:173-225
        DPrim& pr = m->prims[p];
        memset(&pr, 0, sizeof pr);
        pr.vertex_num = (w[0] >> 16) & 0xffff;
        pr.parts_no = w[1] & 0xfff;
        pr.stride = (w[2] >> 16) & 0xff;
        pr.topology = (w[2] >> 24) & 0x3f;
        pr.vertex_base = w[4];
        pr.index_ofs = w[6];
        pr.index_num = w[7];
        pr.index_base = w[8];
        if (pr.topology != 4 && pr.topology != 3)  // PrimitiveTopology::from_repr().unwrap(), src/rmodel.rs:215
            return fail(d, MTR_E_UNSUPPORTED, "primitive " + std::to_string(p) + ": topology " + std::to_string(pr.topology));
        const mtr_layout& l = layouts[p];
        if (l.num_elements > 8) return fail(d, MTR_E_INVALID, "layout has more than 8 elements");
        bool has_pos = false, has_joint = false, has_weight = false;
        uint32_t align_or = pr.vertex_base | pr.stride;
        for (uint32_t i = 0; i < l.num_elements; i++) {
            const mtr_element& e = l.elements[i];
            if (e.format == MTR_IEF_SCMP3N && !(e.flags & MTR_ELEM_DECODE_SCMP3N)) continue;  // src/rshader2.rs:509-512
            if (e.semantic == MTR_SEM_POSITION || e.semantic == MTR_SEM_TEXCOORD) {
                uint32_t nb = elem_bytes(e.format, e.count);
                if (nb == 0)  // todo!() arms of src/rshader2.rs:516-564 and integer formats
                    return fail(d, MTR_E_UNSUPPORTED, "primitive " + std::to_string(p) + ": unhandled element format " +
                                                         std::to_string(e.format) + " x" + std::to_string(e.count));
                if ((uint32_t)e.offset + nb > pr.stride) return fail(d, MTR_E_INVALID, "element outside the vertex stride");
                align_or |= e.offset;
                if (e.semantic == MTR_SEM_POSITION) {
                    has_pos = true; pr.pos_fmt = e.format; pr.pos_cnt = e.count; pr.pos_off = e.offset;
                } else {
                    pr.has_uv = 1; pr.uv_fmt = e.format; pr.uv_cnt = e.count; pr.uv_off = e.offset;
                }
            } else if (e.semantic == MTR_SEM_JOINT) {
                if (e.format != MTR_IEF_U8 || e.count != 4) return fail(d, MTR_E_UNSUPPORTED, "Joint must be U8 x4");
                if ((uint32_t)e.offset + 4 > pr.stride) return fail(d, MTR_E_INVALID, "element outside the vertex stride");
                has_joint = true; pr.joint_off = e.offset; align_or |= e.offset;
            } else if (e.semantic == MTR_SEM_WEIGHT) {
                if (e.format != MTR_IEF_U8N || e.count != 4) return fail(d, MTR_E_UNSUPPORTED, "Weight must be U8N x4");
                if ((uint32_t)e.offset + 4 > pr.stride) return fail(d, MTR_E_INVALID, "element outside the vertex stride");
                has_weight = true; pr.weight_off = e.offset; align_or |= e.offset;
            }  // other names: `_ => continue`, src/rshader2.rs:506
        }
        if (!has_pos) return fail(d, MTR_E_UNSUPPORTED, "primitive " + std::to_string(p) + ": no Position element");
        pr.skinnable = has_joint && has_weight;
        pr.aligned4 = (align_or & 3) == 0;
        if ((size_t)pr.vertex_base + (size_t)pr.vertex_num * pr.stride > vertex_len)
            return fail(d, MTR_E_INVALID, "primitive " + std::to_string(p) + ": vertex slice outside the buffer");
        if ((size_t)pr.index_ofs + pr.index_num > index_num)
            return fail(d, MTR_E_INVALID, "primitive " + std::to_string(p) + ": index range outside the buffer");
        int32_t tex = prim_to_texture ? prim_to_texture[p] : -1;
        if (tex >= (int32_t)ntextures) return fail(d, MTR_E_INVALID, "prim_to_texture out of range");
        m->prim_to_texture[p] = tex < 0 ? -1 : tex;
        uint32_t id = prim_debug_id ? prim_debug_id[p] : 0;
        float c[4];
        for (int k = 0; k < 3; k++) c[k] = (float)kDebugPalette[id % 20][k] / 255.0f;  // debug_ids.wgsl:46
        c[3] = 1.0f;
        m->debug_rgba8[p] = pack_rgba8(c);
    }
    m->parts_disp.assign(nprims, 1);  // src/model.rs:270
    m->indices.resize(index_num);  // the caller's pointer may be an unaligned view into a file image: bytes only
    if (index_num) memcpy(m->indices.data(), index_buf, index_num * sizeof(uint16_t));
    m->run.resize(index_num);
    {
        // runs restart at every primitive's first index so a chunk never looks outside its primitive
        std::vector<uint8_t> is_first(index_num + 1, 0);
        for (auto& pr : m->prims) is_first[pr.index_ofs] = 1;
        uint32_t r = 0;
        for (size_t i = 0; i < index_num; i++) {
            if (is_first[i]) r = 0;
            r = m->indices[i] == 0xFFFF ? 0 : r + 1;
            m->run[i] = r;
        }
    }
    int32_t rc = set_device(d);
    if (rc) return rc;
    if ((rc = dev_alloc(d, &m->d_vbuf, vertex_len + 16))) return rc;
    if ((rc = dev_alloc(d, &m->d_ibuf, index_num + 2))) return rc;
    if ((rc = dev_alloc(d, &m->d_prims, nprims))) return rc;
    {
        std::vector<BoneBox> boxes, inst_boxes;
        build_bounds(m.get(), static_cast<const uint8_t*>(vertex_buf), boxes, inst_boxes);
        if ((rc = dev_alloc(d, &m->d_boxes, boxes.size()))) return rc;
        if ((rc = dev_alloc(d, &m->d_inst_boxes, inst_boxes.size()))) return rc;
        if (!boxes.empty()) HIPCHK(d, hipMemcpy(m->d_boxes, boxes.data(), boxes.size() * sizeof(BoneBox), hipMemcpyHostToDevice));
        if (!inst_boxes.empty()) HIPCHK(d, hipMemcpy(m->d_inst_boxes, inst_boxes.data(), inst_boxes.size() * sizeof(BoneBox), hipMemcpyHostToDevice));
    }
    HIPCHK(d, hipMemcpyAsync(m->d_vbuf, vertex_buf, vertex_len, hipMemcpyHostToDevice, d->stream));
    HIPCHK(d, hipMemcpyAsync(m->d_ibuf, index_buf, index_num * 2, hipMemcpyHostToDevice, d->stream));
    HIPCHK(d, hipMemcpyAsync(m->d_prims, m->prims.data(), nprims * sizeof(DPrim), hipMemcpyHostToDevice, d->stream));
    HIPCHK(d, hipStreamSynchronize(d->stream));
    *out = m.release();
    return MTR_OK;
}

void mtr_model_destroy(mtr_model* m) {
    if (!m) return;
    (void)hipSetDevice(m->dev->hip_dev);
    (void)drain_all(m->dev);  // frames in flight (on any slot stream) may still read its buffers
    for (auto& pb : m->pal_ring) {
        if (pb.d) (void)hipFree(pb.d);
        if (pb.ready) (void)hipEventDestroy(pb.ready);
    }
    if (m->skel.d) (void)hipDeviceSynchronize();  // a pose kernel on a caller's stream may still read the skeleton
    void* ptrs[] = {m->d_vbuf, m->d_ibuf, m->d_prims, m->d_boxes, m->d_inst_boxes, m->skel.d};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    delete m;
}

int32_t mtr_model_set_prim_states(mtr_model* m, const mtr_prim_state* states, size_t nprims) {
    if (!m) return MTR_E_INVALID;
    mtr_device* d = m->dev;
    if (states && nprims != m->prims.size()) return fail(d, MTR_E_INVALID, "one state per primitive");
    for (size_t p = 0; states && p < nprims; p++)
        if (states[p].blend > MTR_BLEND_ADD || states[p].cull > MTR_CULL_FRONT) return fail(d, MTR_E_INVALID, "unknown blend / cull mode");
    int32_t rc = set_device(d);
    if (rc) return rc;
    std::lock_guard<std::mutex> submit_lock(d->submit_mu);
    if (states) m->states.assign(states, states + nprims); else m->states.clear();
    bool changed = false;
    for (size_t p = 0; p < m->prims.size(); p++) {
        const uint32_t cull = states ? states[p].cull : (uint32_t)MTR_CULL_BACK;
        changed = changed || m->prims[p].cull != cull;
        m->prims[p].cull = cull;
    }
    if (changed) {  // the cull mode lives in the device copy of the primitive table: frames in flight may be reading it
        if ((rc = drain_all(d))) return rc;
        HIPCHK(d, hipMemcpy(m->d_prims, m->prims.data(), m->prims.size() * sizeof(DPrim), hipMemcpyHostToDevice));
    }
    return MTR_OK;
}

int32_t mtr_model_set_parts_disp(mtr_model* m, const uint8_t* parts_disp, size_t n) {
    if (!m || (!parts_disp && n)) return MTR_E_INVALID;
    // the exchange thread may be re-running a frame that drew this model: the table a recorded draw holds is immutable,
    // and what the next draw will see changes under the lock
    std::lock_guard<std::mutex> submit_lock(m->dev->submit_mu);
    m->parts_disp.assign(parts_disp, parts_disp + n);
    m->chunks_dirty = true;
    return MTR_OK;
}

int32_t mtr_model_set_palette(mtr_model* m, const float* mats, size_t n) {
    if (!m) return MTR_E_INVALID;
    mtr_device* d = m->dev;
    if (n > 256 || (!mats && n)) return fail(d, MTR_E_INVALID, "palette: at most 256 matrices (u8 joint indices)");
    int32_t rc = set_device(d);
    if (rc) return rc;
    std::lock_guard<std::mutex> submit_lock(d->submit_mu);
    m->npal = (uint32_t)n;
    m->d_palette = nullptr;
    m->pal_ready = nullptr;
    m->pal_slot = -1;
    if (n) {
        mtr_model::PalBuf* pb = nullptr;
        if ((rc = next_palette_buffer(m, n, &pb))) return rc;
        HIPCHK(d, hipMemcpyAsync(pb->d, mats, n * 64, hipMemcpyHostToDevice, d->s_copy));
        HIPCHK(d, hipEventRecord(pb->ready, d->s_copy));
    }
    return MTR_OK;
}

int32_t mtr_model_set_skeleton(mtr_model* m, const uint8_t* parents, const float* imats, size_t njoints) {
    if (!m) return MTR_E_INVALID;
    mtr_device* d = m->dev;
    mtr_model::Skeleton sk{};
    if (parents) {
        if (!imats || njoints == 0 || njoints > MTR_POSE_MAX_JOINTS) return fail(d, MTR_E_INVALID, "skeleton: 1 to 256 joints and their inverse bind matrices");
        std::vector<uint32_t> paths;
        std::vector<uint8_t> bytes;
        if (!pose_paths(parents, njoints, paths, bytes)) return fail(d, MTR_E_INVALID, "skeleton: a parent out of range or a cycle");
        int32_t rc = set_device(d);
        if (rc) return rc;
        std::vector<float> img(njoints * 17 + bytes.size() / 4);  // imats, the path table, the paths (bytes padded to words)
        memcpy(img.data(), imats, njoints * 64);
        memcpy(img.data() + njoints * 16, paths.data(), njoints * 4);
        memcpy(img.data() + njoints * 17, bytes.data(), bytes.size());
        sk.path_bytes = (uint32_t)bytes.size();
        if ((rc = dev_alloc(d, &sk.d, img.size()))) return rc;
        const hipError_t e = hipMemcpy(sk.d, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(sk.d); return fail(d, MTR_E_HIP, std::string("hipMemcpy: ") + hipGetErrorString(e)); }
        sk.njoints = (uint32_t)njoints;
        sk.parents.assign(parents, parents + njoints);
        for (size_t j = 0; j < njoints; j++)
            if (sk.parents[j] == j) sk.parents[j] = 255;  // a root either way
    }
    mtr_model::Skeleton old;
    {
        std::lock_guard<std::mutex> submit_lock(d->submit_mu);
        old = m->skel;
        m->skel = sk;
    }
    if (old.d) {  // a pose kernel (on s_copy or a caller's stream) may still read it; skeletons change at set-up, not per frame
        (void)hipDeviceSynchronize();
        (void)hipFree(old.d);
    }
    return MTR_OK;
}

int32_t mtr_model_set_pose(mtr_model* m, const float* local_mats, size_t njoints) {
    if (!m) return MTR_E_INVALID;
    mtr_device* d = m->dev;
    if (!m->skel.d) return fail(d, MTR_E_INVALID, "pose: the model has no skeleton");
    if (!local_mats || njoints != m->skel.njoints) return fail(d, MTR_E_INVALID, "pose: one local matrix per joint of the skeleton");
    if (!mtr_launch_pose) return fail(d, MTR_E_UNSUPPORTED, "pose: built without k_pose");
    int32_t rc = set_device(d);
    if (rc) return rc;
    if ((rc = stage_pose(d, local_mats, njoints * 16))) return rc;
    std::lock_guard<std::mutex> submit_lock(d->submit_mu);
    mtr_model::PalBuf* pb = nullptr;
    if ((rc = next_palette_buffer(m, njoints, &pb))) return rc;
    mtr_launch_pose(pose_params(m->skel, d->pose_stage, pb->d), 1, d->s_copy);
    HIPCHK(d, hipGetLastError());
    HIPCHK(d, hipEventRecord(pb->ready, d->s_copy));
    return MTR_OK;
}

int32_t mtr_model_set_joint_positions(mtr_model* m, const float* xyz, size_t n) {
    if (!m || (!xyz && n)) return MTR_E_INVALID;
    if (n > 0xFFFF) return fail(m->dev, MTR_E_INVALID, "too many joints");
    m->joint_cubes.assign(n * 16, 0.0f);
    for (size_t j = 0; j < n; j++) {
        float* M = &m->joint_cubes[j * 16];  // glam::Mat4::from_scale_rotation_translation(splat(0.005), IDENTITY, pos * 0.01)
        M[0] = M[5] = M[10] = 0.005f;
        M[12] = xyz[3 * j + 0] * 0.01f; M[13] = xyz[3 * j + 1] * 0.01f; M[14] = xyz[3 * j + 2] * 0.01f;
        M[15] = 1.0f;
    }
    return MTR_OK;
}

int32_t mtr_model_vertex_stage(mtr_model* m, size_t prim, const float M[16], float* out_clip, float* out_uv) {
    if (!m || !M || !out_clip || !out_uv) return MTR_E_INVALID;
    mtr_device* d = m->dev;
    if (prim >= m->prims.size()) return fail(d, MTR_E_INVALID, "primitive out of range");
    int32_t rc = set_device(d);
    if (rc) return rc;
    const uint32_t nv = m->prims[prim].vertex_num;
    if (nv == 0) return MTR_OK;
    float *d_clip = nullptr, *d_uv = nullptr;
    if ((rc = dev_alloc(d, &d_clip, (size_t)nv * 4))) return rc;
    if ((rc = dev_alloc(d, &d_uv, (size_t)nv * 2))) return rc;
    GeomParams gp{};
    gp.vbuf = m->d_vbuf; gp.ibuf = m->d_ibuf; gp.prims = m->d_prims; gp.ninst = 1;
    gp.palettes = m->d_palette; gp.npal = m->d_palette ? m->npal : 0;
    memcpy(gp.vp, M, sizeof gp.vp);
    if (m->pal_ready) HIPCHK(d, hipStreamWaitEvent(d->stream, m->pal_ready, 0));
    mtr_launch_vertex_stage(gp, (uint32_t)prim, d_clip, d_uv, d->stream);
    HIPCHK(d, hipGetLastError());
    HIPCHK(d, hipMemcpyAsync(out_clip, d_clip, (size_t)nv * 16, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(d, hipMemcpyAsync(out_uv, d_uv, (size_t)nv * 8, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(d, hipStreamSynchronize(d->stream));
    (void)hipFree(d_clip);
    (void)hipFree(d_uv);
    return MTR_OK;
}

}  // extern "C"
