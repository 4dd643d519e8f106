// The image entry points of the extern "C" shim (include/tungsten_hip.h): the transfers of the framebuffer, the SampleRecords, the auxiliary outputs
// and the per-sample radiance between the context and the caller's host memory, tghip_develop and tghip_nlmeans with their getters.  Host code only:
// the kernels are behind the launchers of develop.h and denoise.h, the context and what the shim's units share are shim_context.h's.
#include "shim_context.h"
#include "denoise.h"
#include "develop.h"
#include <cstring>

// What the seven transfers do behind their argument checks, once the pass under way has run out (runOutPass): the device, one or two copies of
// `bytes` bytes from src to dst on the context's stream (dst == nullptr: an array the caller does not ask for), the stream run dry
struct Transfer { void *dst; const void *src; size_t bytes; };
static int transfer(tghip_ctx *ctx, hipMemcpyKind kind, const Transfer &a, const Transfer &b = Transfer{nullptr, nullptr, 0})
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (a.dst) HIP_TRY(ctx, hipMemcpyAsync(a.dst, a.src, a.bytes, kind, ctx->stream));
    if (b.dst) HIP_TRY(ctx, hipMemcpyAsync(b.dst, b.src, b.bytes, kind, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TGHIP_OK;
}

extern "C" {

int tghip_download_framebuffer(tghip_ctx *ctx, float *rgb_sum, uint32_t *count, size_t npixels)
{
    if (!ctx || !ctx->haveScene) return TGHIP_E_NOSCENE;
    if (npixels != size_t(ctx->width)*ctx->height) { ctx->error = "pixel count mismatch"; return TGHIP_E_INVALID; }
    if (const int rc = runOutPass(ctx); rc != TGHIP_OK) return rc;
    return transfer(ctx, hipMemcpyDeviceToHost, {rgb_sum, ctx->frameSum(), npixels*3*sizeof(float)}, {count, ctx->frameCount(), npixels*sizeof(uint32_t)});
}

int tghip_upload_framebuffer(tghip_ctx *ctx, const float *rgb_sum, const uint32_t *count, size_t npixels)
{
    if (!ctx || !ctx->haveScene) return TGHIP_E_NOSCENE;
    if (!rgb_sum || !count || npixels != size_t(ctx->width)*ctx->height) { ctx->error = "pixel count mismatch"; return TGHIP_E_INVALID; }
    if (const int rc = runOutPass(ctx); rc != TGHIP_OK) return rc;
    return transfer(ctx, hipMemcpyHostToDevice, {ctx->frameSum(), rgb_sum, npixels*3*sizeof(float)}, {ctx->frameCount(), count, npixels*sizeof(uint32_t)});
}

int tghip_download_records(tghip_ctx *ctx, TgHipSampleRecord *out, size_t n)
{
    if (!ctx || !ctx->haveScene) return TGHIP_E_NOSCENE;
    if (!out || n != size_t((ctx->width + 3)/4)*((ctx->height + 3)/4)) { ctx->error = "record count mismatch"; return TGHIP_E_INVALID; }
    if (const int rc = runOutPass(ctx); rc != TGHIP_OK) return rc;
    return transfer(ctx, hipMemcpyDeviceToHost, {out, ctx->dRecords, n*sizeof(TgHipSampleRecord)});
}

int tghip_upload_records(tghip_ctx *ctx, const TgHipSampleRecord *in, size_t n)
{
    if (!ctx || !ctx->haveScene) return TGHIP_E_NOSCENE;
    if (!in || n != size_t((ctx->width + 3)/4)*((ctx->height + 3)/4)) { ctx->error = "record count mismatch"; return TGHIP_E_INVALID; }
    if (const int rc = runOutPass(ctx); rc != TGHIP_OK) return rc;
    return transfer(ctx, hipMemcpyHostToDevice, {ctx->dRecords, in, n*sizeof(TgHipSampleRecord)});
}

int tghip_download_aux(tghip_ctx *ctx, TgHipAuxPixel *out, size_t npixels)
{
    if (!ctx || !ctx->haveScene) return TGHIP_E_NOSCENE;
    if (!out || npixels != size_t(ctx->width)*ctx->height) { ctx->error = "pixel count mismatch"; return TGHIP_E_INVALID; }
    if (const int rc = runOutPass(ctx); rc != TGHIP_OK) return rc;
    if (!ctx->dAux) { std::memset(out, 0, npixels*sizeof(TgHipAuxPixel)); return TGHIP_OK; }   // no TGHIP_PASS_AUX pass yet
    return transfer(ctx, hipMemcpyDeviceToHost, {out, ctx->dAux.get(), npixels*sizeof(TgHipAuxPixel)});
}

int tghip_upload_aux(tghip_ctx *ctx, const TgHipAuxPixel *in, size_t npixels)
{
    if (!ctx || !ctx->haveScene) return TGHIP_E_NOSCENE;
    if (!in || npixels != size_t(ctx->width)*ctx->height) { ctx->error = "pixel count mismatch"; return TGHIP_E_INVALID; }
    int rc = runOutPass(ctx);
    if (rc != TGHIP_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));     // (for the allocation: no TGHIP_PASS_AUX pass has made the buffers yet)
    if (!ctx->dAux && (rc = ctx->dAux.grow(ctx, npixels)) != TGHIP_OK) return rc;
    return transfer(ctx, hipMemcpyHostToDevice, {ctx->dAux.get(), in, npixels*sizeof(TgHipAuxPixel)});
}

int tghip_download_samples(tghip_ctx *ctx, float *rgb, size_t nfloats)
{
    if (!ctx || !ctx->haveScene) return TGHIP_E_NOSCENE;
    if (const int rc = runOutPass(ctx); rc != TGHIP_OK) return rc;
    if (!rgb || !ctx->dSamples || nfloats != ctx->samplesFloats) { ctx->error = "no TGHIP_PASS_SAMPLES pass of that size has been rendered"; return TGHIP_E_INVALID; }
    return transfer(ctx, hipMemcpyDeviceToHost, {rgb, ctx->dSamples.get(), nfloats*sizeof(float)});
}

int tghip_develop(tghip_ctx *ctx, const TgHipDevelopDesc *desc, float *hdr_out, uint8_t *ldr_out, size_t npixels)
{
    if (!ctx) return TGHIP_E_INVALID;
    if (!desc) { ctx->error = "tghip_develop: no description"; return TGHIP_E_INVALID; }
    if (!ctx->haveScene) { ctx->error = "tghip_develop before tghip_upload_scene"; return TGHIP_E_NOSCENE; }
    const bool frame = desc->source == TGHIP_DEVELOP_FRAME;
    if (!frame && desc->source >= TGHIP_AUX_OUTPUTS) { ctx->error = "tghip_develop: unknown source"; return TGHIP_E_INVALID; }
    if (desc->part > TGHIP_DEVELOP_VARIANCE) { ctx->error = "tghip_develop: unknown part"; return TGHIP_E_INVALID; }
    if (frame && desc->tonemap > TGHIP_TONEMAP_PBRT) { ctx->error = "tghip_develop: unknown tone-mapping operator"; return TGHIP_E_INVALID; }
    if (frame && desc->part != TGHIP_DEVELOP_MEAN) { ctx->error = "tghip_develop: the framebuffer has no A / B halves and no variance"; return TGHIP_E_INVALID; }
    if (npixels != size_t(ctx->width)*ctx->height) { ctx->error = "pixel count mismatch"; return TGHIP_E_INVALID; }
    if (ctx->developHost) { ctx->error = "tghip_develop: the develop_host option is set (the caller develops on the host)"; return TGHIP_E_UNSUPPORTED; }
    int rc = runOutPass(ctx);
    if (rc != TGHIP_OK) return rc;
    if (!frame && !ctx->dAux) { ctx->error = "tghip_develop: no auxiliary output buffers yet (no TGHIP_PASS_AUX pass, no tghip_upload_aux)"; return TGHIP_E_INVALID; }
    const float *sum = ctx->frameSum();
    const uint32_t *cnt = ctx->frameCount();
    if (frame && ((reinterpret_cast<uintptr_t>(sum) | reinterpret_cast<uintptr_t>(cnt)) & 15u)) { ctx->error = "tghip_develop: the bound framebuffer is not 16-byte aligned"; return TGHIP_E_INVALID; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t hdrFloats = npixels*(frame || (desc->source != TGHIP_AUX_DEPTH && desc->source != TGHIP_AUX_VISIBILITY) ? 3 : 1);
    const bool device = (desc->flags & TGHIP_DEVELOP_DEVICE_POINTERS) != 0;
    if (device && ((reinterpret_cast<uintptr_t>(hdr_out) & 15u) || (reinterpret_cast<uintptr_t>(ldr_out) & 3u))) { ctx->error = "tghip_develop: device outputs must be aligned (hdr_out to 16 bytes, ldr_out to 4)"; return TGHIP_E_INVALID; }
    float *hdr = nullptr;
    uint8_t *ldr = nullptr;
    if ((rc = stageOutput(ctx, device, hdr_out, hdrFloats*sizeof(float), ctx->developHdr, hdr)) != TGHIP_OK) return rc;
    if ((rc = stageOutput(ctx, device, ldr_out, npixels*3, ctx->developLdr, ldr)) != TGHIP_OK) return rc;
    HIP_TRY(ctx, ctx->developMax.once(16));
    return timedLaunches(ctx, ctx->developMs, [&]() -> int {
        if (frame) HIP_TRY(ctx, developLaunchFrame(ctx->stream, sum, cnt, npixels, desc->tonemap, hdr, ldr));
        else HIP_TRY(ctx, developLaunchAux(ctx->stream, ctx->dAux.get(), npixels, desc->source, desc->part, hdr, ldr, ctx->developMax.get()));
        return TGHIP_OK;
    }, [&]() -> int {
        const int crc = copyBack(ctx, hdr_out, hdr, hdrFloats*sizeof(float));
        return crc != TGHIP_OK ? crc : copyBack(ctx, ldr_out, ldr, npixels*3);
    });
}

int tghip_develop_kernel_time(tghip_ctx *ctx, double *ms) { return kernelTime(ctx, &tghip_ctx::developMs, ms); }

int tghip_nlmeans(tghip_ctx *ctx, const TgHipNlMeansDesc *desc, const float *image, const float *guide, const float *variance, float *out)
{
    if (!ctx) return TGHIP_E_INVALID;
    if (!desc) { ctx->error = "tghip_nlmeans: no description"; return TGHIP_E_INVALID; }
    const bool pointers = desc->source == TGHIP_NLMEANS_POINTERS;
    if (!pointers && desc->source >= TGHIP_AUX_OUTPUTS) { ctx->error = "tghip_nlmeans: unknown source"; return TGHIP_E_INVALID; }
    uint32_t channels = desc->channels;
    if (!pointers) channels = (desc->source == TGHIP_AUX_DEPTH || desc->source == TGHIP_AUX_VISIBILITY) ? 1 : 3;
    if (channels < 1 || channels > 4) { ctx->error = "tghip_nlmeans: channels must be 1..4"; return TGHIP_E_INVALID; }
    if (desc->F > NLMEANS_MAX_F) { ctx->error = "tghip_nlmeans: F must be 0..8"; return TGHIP_E_INVALID; }
    if (desc->R > NLMEANS_MAX_R) { ctx->error = "tghip_nlmeans: R must be 0..16"; return TGHIP_E_INVALID; }
    if (!(desc->k > 0.0f)) { ctx->error = "tghip_nlmeans: k must be positive"; return TGHIP_E_INVALID; }
    if (desc->width == 0 || desc->height == 0) { ctx->error = "tghip_nlmeans: the image has no pixels"; return TGHIP_E_INVALID; }
    if (desc->width > (1u << 20) || desc->height > (1u << 20)) { ctx->error = "tghip_nlmeans: the image is too large"; return TGHIP_E_INVALID; }
    if (!out) { ctx->error = "tghip_nlmeans: no output array"; return TGHIP_E_INVALID; }
    if (pointers && (!image || !guide || !variance)) { ctx->error = "tghip_nlmeans: image, guide and variance are needed without an aux source"; return TGHIP_E_INVALID; }
    if (!pointers && (image || guide || variance)) { ctx->error = "tghip_nlmeans: an aux source takes no image, guide or variance pointers"; return TGHIP_E_INVALID; }
    if (!pointers && (desc->image_part > TGHIP_DEVELOP_B || desc->guide_part > TGHIP_DEVELOP_B)) { ctx->error = "tghip_nlmeans: image_part and guide_part are the mean or a half"; return TGHIP_E_INVALID; }
    int rc = runOutPass(ctx);
    if (rc != TGHIP_OK) return rc;
    if (!pointers && (!ctx->haveScene || !ctx->dAux)) { ctx->error = "tghip_nlmeans: no auxiliary output buffers yet (no TGHIP_PASS_AUX pass, no tghip_upload_aux)"; return TGHIP_E_INVALID; }
    if (!pointers && (desc->width != uint32_t(ctx->width) || desc->height != uint32_t(ctx->height))) { ctx->error = "tghip_nlmeans: an aux source has the frame's size"; return TGHIP_E_INVALID; }
    const bool device = (desc->flags & TGHIP_DEVELOP_DEVICE_POINTERS) != 0;
    const uintptr_t align = channels == 4 ? 15u : 3u;
    if (device) {
        const uintptr_t all = reinterpret_cast<uintptr_t>(image) | reinterpret_cast<uintptr_t>(guide) | reinterpret_cast<uintptr_t>(variance) | reinterpret_cast<uintptr_t>(out);
        if (all & align) { ctx->error = "tghip_nlmeans: device arrays must be aligned (to 16 bytes with four channels, to 4 otherwise)"; return TGHIP_E_INVALID; }
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t npixels = size_t(desc->width)*desc->height, nfloats = npixels*channels, nbytes = nfloats*sizeof(float);
    // scratch planes 0..2: image, guide, variance (uploaded, or developed from the aux buffers); 3: the result of a call with host memory
    const float *in[3] = {image, guide, variance};
    float *result = nullptr;
    for (int b = 0; b < 3; ++b) {
        if (pointers) rc = stageInput(ctx, device, in[b], nbytes, ctx->nlmBuf[b], in[b]);
        else { rc = ctx->nlmBuf[b].grow(ctx, nfloats); in[b] = ctx->nlmBuf[b].get(); }   // (developed below)
        if (rc != TGHIP_OK) return rc;
    }
    if ((rc = stageOutput(ctx, device, out, nbytes, ctx->nlmBuf[3], result)) != TGHIP_OK) return rc;
    return timedLaunches(ctx, ctx->nlmMs, [&]() -> int {
        if (!pointers) {
            HIP_TRY(ctx, ctx->developMax.once(16));
            const uint32_t parts[3] = {desc->image_part, desc->guide_part, TGHIP_DEVELOP_VARIANCE};
            for (int b = 0; b < 3; ++b)
                HIP_TRY(ctx, developLaunchAux(ctx->stream, ctx->dAux.get(), npixels, desc->source, parts[b], ctx->nlmBuf[b].get(), nullptr, ctx->developMax.get()));
        }
        HIP_TRY(ctx, nlMeansLaunch(ctx->stream, in[0], in[1], in[2], result, desc->width, desc->height, channels, desc->F, desc->R, desc->k,
                                   desc->variance_scale, ctx->nlmBatch));
        return TGHIP_OK;
    }, [&]() { return copyBack(ctx, out, result, nbytes); });
}

int tghip_nlmeans_kernel_time(tghip_ctx *ctx, double *ms) { return kernelTime(ctx, &tghip_ctx::nlmMs, ms); }

} // extern "C"
