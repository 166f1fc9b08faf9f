// host_texture.cpp -- textures: upload, BC decode at creation, residency.
#include "host.h"

using namespace mtr_host;

extern "C" {

// ---------------------------------------------------------------------------------------------
// Texture::new
// ---------------------------------------------------------------------------------------------
int32_t mtr_texture_create_mips(mtr_device* d, uint32_t w, uint32_t h, uint32_t fmt, uint32_t levels, const void* data, size_t len,
                                mtr_texture** out) {
    if (!d || !out) return MTR_E_INVALID;
    *out = nullptr;
    if (!data || w == 0 || h == 0 || w > 16384 || h > 16384) return fail(d, MTR_E_INVALID, "bad texture size/data");
    if (levels == 0 || levels > 15 || (levels > 1 && (w >> (levels - 1)) == 0 && (h >> (levels - 1)) == 0))
        return fail(d, MTR_E_INVALID, "more mip levels than the texture size allows");
    if (fmt != MTR_TEX_RGBA8 && fmt != MTR_TEX_BC1 && fmt != MTR_TEX_BC7 && fmt != MTR_TEX_BC7_ALT)
        return fail(d, MTR_E_UNSUPPORTED, "unhandled texture format " + std::to_string(fmt));  // src/rtexture.rs:159
    // level l: max(1, w >> l) x max(1, h >> l), stored level after level in both the source and the decoded image
    size_t need = 0, texels = 0;
    for (uint32_t l = 0; l < levels; l++) {
        const size_t lw = std::max(1u, w >> l), lh = std::max(1u, h >> l);
        need += fmt == MTR_TEX_RGBA8 ? lw * lh * 4 : ((lw + 3) / 4) * ((lh + 3) / 4) * (fmt == MTR_TEX_BC1 ? 8 : 16);
        texels += lw * lh;
    }
    if (len < need) return fail(d, MTR_E_INVALID, "texture data too short");
    int32_t rc = set_device(d);
    if (rc) return rc;
    auto t = std::make_unique<mtr_texture>();
    t->dev = d; t->w = w; t->h = h; t->fmt = fmt; t->levels = levels; t->d_rgba = nullptr;
    uint8_t* d_rgba = nullptr;    // the decoded image: the resident one, or (blocks resident) a temporary for the alpha scan
    uint8_t* d_blocks = nullptr;
    const bool keep_blocks = fmt != MTR_TEX_RGBA8 && d->texture_residency == MTR_TEXRES_BLOCKS;
    rc = dev_alloc(d, &d_rgba, texels * 4);
    if (rc) return rc;
    if (fmt == MTR_TEX_RGBA8) {
        HIPCHK(d, hipMemcpyAsync(d_rgba, data, need, hipMemcpyHostToDevice, d->stream));
        HIPCHK(d, hipStreamSynchronize(d->stream));
    } else {
        rc = dev_alloc(d, &d_blocks, need);
        if (rc) { (void)hipFree(d_rgba); return rc; }
        HIPCHK(d, hipMemcpyAsync(d_blocks, data, need, hipMemcpyHostToDevice, d->stream));
        size_t src_off = 0, dst_off = 0;
        for (uint32_t l = 0; l < levels; l++) {
            const uint32_t lw = std::max(1u, w >> l), lh = std::max(1u, h >> l);
            if (fmt == MTR_TEX_BC1) mtr_launch_bc1_decode(d_blocks + src_off, d_rgba + dst_off, lw, lh, d->stream);
            else mtr_launch_bc7_decode(d_blocks + src_off, d_rgba + dst_off, lw, lh, d->stream);
            src_off += (size_t)((lw + 3) / 4) * ((lh + 3) / 4) * (fmt == MTR_TEX_BC1 ? 8 : 16);
            dst_off += (size_t)lw * lh * 4;
        }
        HIPCHK(d, hipGetLastError());
        HIPCHK(d, hipStreamSynchronize(d->stream));
    }
    {
        uint32_t* d_min = nullptr;
        uint32_t h_min = 255;
        if ((rc = dev_alloc(d, &d_min, 1))) return rc;
        HIPCHK(d, hipMemcpyAsync(d_min, &h_min, 4, hipMemcpyHostToDevice, d->stream));
        mtr_launch_alpha_min(d_rgba, texels, d_min, d->stream);
        HIPCHK(d, hipGetLastError());
        HIPCHK(d, hipMemcpyAsync(&h_min, d_min, 4, hipMemcpyDeviceToHost, d->stream));
        HIPCHK(d, hipStreamSynchronize(d->stream));
        (void)hipFree(d_min);
        t->opaque = h_min == 255;
    }
    if (keep_blocks) {  // the sampler decodes the texel's block per fetch (csrc/bc_sample.h): 1/4 (BC7) or 1/8 (BC1) of the bytes
        (void)hipFree(d_rgba);
        t->d_rgba = d_blocks;
        t->resident = fmt == MTR_TEX_BC1 ? MTR_TR_BC1 : MTR_TR_BC7;
    } else {
        if (d_blocks) (void)hipFree(d_blocks);
        t->d_rgba = d_rgba;
    }
    *out = t.release();
    return MTR_OK;
}

int32_t mtr_texture_create(mtr_device* d, uint32_t w, uint32_t h, uint32_t fmt, const void* data, size_t len, mtr_texture** out) {
    return mtr_texture_create_mips(d, w, h, fmt, 1, data, len, out);
}

void mtr_texture_destroy(mtr_texture* t) {
    if (!t) return;
    (void)hipSetDevice(t->dev->hip_dev);
    (void)drain_all(t->dev);  // frames in flight (on any slot stream) may still sample it
    (void)hipFree(t->d_rgba);
    delete t;
}

int32_t mtr_texture_read_rgba8(mtr_texture* t, void* out, size_t len) {
    if (!t || !out) return MTR_E_INVALID;
    mtr_device* d = t->dev;
    if (len < (size_t)t->w * t->h * 4) return fail(d, MTR_E_INVALID, "output too small");
    if (t->resident != MTR_TR_RGBA8) return fail(d, MTR_E_UNSUPPORTED, "the texture is resident as BC blocks (mtr_device_set_texture_residency): there is no decoded image to read");
    int32_t rc = set_device(d);
    if (rc) return rc;
    HIPCHK(d, hipMemcpyAsync(out, t->d_rgba, (size_t)t->w * t->h * 4, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(d, hipStreamSynchronize(d->stream));
    return MTR_OK;
}

}  // extern "C"
