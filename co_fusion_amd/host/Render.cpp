// Render.cpp -- CoFusion's scene rendering: the models of the map drawn into one view through cf_render (csrc/render.hip), the way the
// reference's viewer draws them (GUI/MainController.cpp:570-600: objects placed by view * globalPose * modelPose^-1), and the
// head-less view export of MainController.cpp:209-214,394-407 (-el / -en / -ev: Labels<n>.png, Normals<n>.png, Viewport<n>.png).
#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "CoFusion.h"
#include "ExportWriter.h"

namespace cofusion {

static void rcheck(cf_ctx* ctx, int rc, const char* what)
{
    if (rc != CF_OK) throw std::runtime_error(std::string(what) + " failed (" + std::to_string(rc) + "): " + (ctx ? cf_last_error(ctx) : ""));
}

void CoFusion::releaseRenderer()
{
    if (renderer) cf_render_destroy(renderer);
    if (renderImages) cf_free(ctx, renderImages);
    renderer = nullptr; renderImages = nullptr; renderW = renderH = 0;
}

// one render object and one set of owned images for views up to renderW x renderH (created at first use, grown when needed)
void CoFusion::ensureRenderer(int w, int h)
{
    if (renderer && w <= renderW && h <= renderH) return;
    const int W = std::max(w, renderW), H = std::max(h, renderH);
    releaseRenderer();
    rcheck(ctx, cf_render_create(ctx, W, H, &renderer), "cf_render_create");
    void* p = nullptr;
    rcheck(ctx, cf_malloc(ctx, (uint64_t)W * H * (3 * 4 + 4 + 1), &p), "render images");
    renderImages = static_cast<uint8_t*>(p);
    renderW = W; renderH = H;
}

cf_render_view CoFusion::currentView() const
{
    cf_render_view v{};
    const Mat4f& p = globalModel->getPose();
    for (int i = 0; i < 16; i++) v.pose[i] = p.m[i];
    v.fx = cfg.fx; v.fy = cfg.fy; v.cx = cfg.cx; v.cy = cfg.cy;
    v.width = cfg.width; v.height = cfg.height;
    return v;
}

void CoFusion::renderScene(const cf_render_view* view, int backgroundMode, int objectMode, int flags, const cf_render_output* outputs, int n)
{
    if (dist.active()) throw std::runtime_error("renderScene: rendering across ranks (model-parallel / sharded background operation) is not supported");
    if (!globalModel) throw std::runtime_error("renderScene: no map yet");
    cf_render_view v = view ? *view : currentView();
    v.flags = flags; v.tick = tick; v.time_delta = cfg.timeDelta;
    ensureRenderer(v.width, v.height);
    std::vector<cf_render_item> items;
    const Mat4f& global = globalModel->getPose();
    for (auto& model : models) {   // (the background heads the list)
        cf_render_item it{};
        void* ptr = nullptr; uint64_t bytes = 0;
        rcheck(ctx, cf_model_buffer(model->handle(), 11, &ptr, &bytes), "cf_model_buffer");
        it.surfels = static_cast<const float*>(ptr);
        it.count = (uint32_t)(bytes / 48);
        const bool bg = model.get() == globalModel.get();
        const Mat4f Tp = bg ? Mat4f::identity() : global * model->getPose().inverse();   // (Export.cpp's Tp)
        for (int i = 0; i < 16; i++) it.pose[i] = Tp.m[i];
        it.conf_threshold = model->getConfidenceThreshold();
        it.model_id = (int)model->getID();
        it.colour_mode = bg ? backgroundMode : objectMode;
        items.push_back(it);
    }
    rcheck(ctx, cf_render(renderer, &v, items.data(), (int)items.size(), outputs, n), "cf_render");
}

void CoFusion::renderSceneOwned(const cf_render_view* view, int backgroundMode, int objectMode, int flags, const uint8_t** rgba,
                                const float** depth, const uint8_t** labels, int* width, int* height)
{
    const int w = view ? view->width : cfg.width, h = view ? view->height : cfg.height;
    if (w <= 0 || h <= 0) throw std::runtime_error("renderScene: empty view");
    ensureRenderer(w, h);
    const size_t N = (size_t)renderW * renderH;
    uint8_t* img = renderImages;
    float* dep = reinterpret_cast<float*>(renderImages + N * 12);
    uint8_t* lab = renderImages + N * 16;
    const cf_render_output outs[3] = {{img, CF_RENDER_RGBA, CF_RENDER_ITEM_MODE}, {dep, CF_RENDER_DEPTH, 0}, {lab, CF_RENDER_LABELS, 0}};
    renderScene(view, backgroundMode, objectMode, flags, outs, 3);
    if (rgba) *rgba = img;
    if (depth) *depth = dep;
    if (labels) *labels = lab;
    if (width) *width = w;
    if (height) *height = h;
}

void CoFusion::setExportViews(const std::string& prefix, int which)
{
    if (which & ~(ExportLabels | ExportNormals | ExportViewport)) throw std::runtime_error("setExportViews: which = 1 labels | 2 normals | 4 viewport");
    if (which && dist.active()) throw std::runtime_error("setExportViews: rendering across ranks (model-parallel / sharded background operation) is not supported");
    exportViewsPrefix = prefix;
    exportViewsWhich = prefix.empty() ? 0 : which;
}

void CoFusion::setExportAsync(bool on, int workers, int slots)
{
    if (exportWriter) { std::unique_ptr<ExportWriter> old = std::move(exportWriter); old->flush(); }   // (off, whatever the flush reports)
    if (on) exportWriter.reset(new ExportWriter(ctx, cfg.width, cfg.height, workers, slots));
}

void CoFusion::exportFlush()
{
    if (exportWriter) exportWriter->flush();
}

void CoFusion::exportStats(uint64_t* images, uint64_t* bytes, uint64_t* stalls, double* deviceMs, uint64_t* deviceImages, bool timing)
{
    ExportWriter::Stats s;
    if (exportWriter) s = exportWriter->stats(timing);
    if (images) *images = s.images;
    if (bytes) *bytes = s.bytes;
    if (stalls) *stalls = s.stalls;
    if (deviceMs) *deviceMs = s.deviceMs;
    if (deviceImages) *deviceImages = s.deviceImages;
}

// after a processed frame: one rasterisation from the current camera feeds the requested colour images
void CoFusion::exportViews(int frameTick)
{
    ensureRenderer(cfg.width, cfg.height);
    const size_t N = (size_t)renderW * renderH;
    const struct { int bit; const char* name; int mode; } kinds[3] = {
        {ExportLabels, "Labels", CF_RENDER_ITEM_MODE}, {ExportNormals, "Normals", CF_RENDER_NORMALS}, {ExportViewport, "Viewport", CF_RENDER_COLOUR}};
    cf_render_output outs[3];
    int n = 0;
    for (auto& k : kinds)
        if (exportViewsWhich & k.bit) {
            outs[n] = cf_render_output{renderImages + N * 4 * n, CF_RENDER_RGBA, k.mode};
            n++;
        }
    renderScene(nullptr, CF_RENDER_COLOUR, CF_RENDER_LABEL, 0, outs, n);
    const size_t frame = (size_t)cfg.width * cfg.height * 4;
    int j = 0;
    if (exportWriter) {   // setExportAsync: encoded on the device, in stream order behind the rasterisation; nothing is read back here
        for (auto& k : kinds)
            if (exportViewsWhich & k.bit)
                exportWriter->submit(exportViewsPrefix + k.name + std::to_string(frameTick) + ".png", outs[j++].dst, cfg.width, cfg.height, 4, 0);
        return;
    }
    std::vector<uint8_t> host(frame);
    for (auto& k : kinds) {
        if (!(exportViewsWhich & k.bit)) continue;
        rcheck(ctx, cf_memcpy_d2h(ctx, host.data(), outs[j++].dst, frame), "exported view readback");
        const std::string path = exportViewsPrefix + k.name + std::to_string(frameTick) + ".png";
        if (!writePngRGBA8(path, host.data(), cfg.width, cfg.height)) throw std::runtime_error("exportViews: cannot write " + path);
    }
}

}  // namespace cofusion
