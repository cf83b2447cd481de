// CoFusion.h -- host-side C++ facade with the reference's class/method names over the C-ABI
// (include/cofusion_hip.h).  This is the layer a maintainer of martinruenz/co-fusion would keep:
//   CoFusion  <- Core/CoFusion.h:44-391      (frame orchestrator, model list, spawn/deactivate)
//   Model     <- Core/Model/Model.h:51-285   (per-model surfel map + tracker)
//   Segmentation <- Core/Segmentation/Segmentation.h:30-140
// Eigen/OpenCV/Pangolin types are replaced by plain structs: poses are ROW-major float[16] (Mat4f),
// images are {pointer,width,height} views.  Only host logic lives here; every per-pixel / per-surfel
// operation is a call into the HIP library.
#pragma once

#include <cstdint>
#include <cstdlib>
#include <functional>
#include <list>
#include <memory>
#include <string>
#include <vector>

#include "../../include/cofusion_hip.h"

namespace cofusion {

struct Mat4f {
    float m[16];
    static Mat4f identity();
    Mat4f inverse() const;             // affine inverse, linear part by cofactors (f32)
    Mat4f operator*(const Mat4f& o) const;
};

// Core/FrameData.h:25-42 (host views; rgb is 3 bytes/pixel R,G,B; depth metres f32; mask u8 or null)
struct FrameData {
    int64_t timestamp = 0;
    const uint8_t* rgb = nullptr;
    const float* depth = nullptr;
    const uint8_t* mask = nullptr;
    // optional: the same frame already resident in HBM (depth f32, rgba u8x4); skips the upload
    const float* depth_dev = nullptr;
    const uint8_t* rgba_dev = nullptr;
    // optional, with a device-resident frame: its label mask in HBM (u8, 16-byte aligned): the mask branch of the segmentation as kernels
    const uint8_t* mask_dev = nullptr;
};

struct SegmentationResult {
    struct ModelData {
        unsigned id = 0;
        int modelIndex = -1;  // position in the model list when the segmentation ran (-1: new label)
        unsigned superPixelCount = 0;
        float avgConfidence = 0, depthMean = 0, depthStd = 0;
        int top = 65535, right = 0, bottom = 0, left = 65535;
    };
    bool hasNewLabel = false;
    float depthRange = 0;
    std::vector<ModelData> modelData;
    std::vector<uint8_t> lowMap;  // 40x30 labels after component analysis (255 = rejected)
};

class CoFusion;
// binary little-endian PLY of an indexed mesh (Mesh.cpp): x y z nx ny nz red green blue | list uchar int vertex_indices
bool writeMeshPly(const std::string& path, const cf_mesh_vertex* vertices, uint32_t nVertices, const uint32_t* triangles, uint32_t nTriangles);
class EnqueuePool;

// host wall-clock per phase of processFrame (diagnostics: where the host keeps the GPU waiting)
struct PhaseTimes {
    enum { Prepare, Track, SegSlicAccumulate, SegUnary, SegCrf, SegPost, ModelLogic, Fuse, Predict, Count };
    double ms[Count] = {0};
    long frames = 0;
};
PhaseTimes& phaseTimes();
// 8-bit greyscale PNG (zlib), Export.cpp
bool writePngGray8(const std::string& path, const uint8_t* data, int width, int height);
// 8-bit RGBA PNG, the same writer (Render.cpp: the exported views)
bool writePngRGBA8(const std::string& path, const uint8_t* data, int width, int height);

// Model-parallel operation over several GPUs (one process per GPU): every rank runs the same frame loop and takes the
// same decisions; a model's surfel map and tracker live only on its owner rank, the other ranks keep a data-less
// shadow.  What crosses ranks -- poses and tracking statistics after tracking, per-superpixel ICP-error / confidence
// sums before the CRF, surfel counts when a model is retired -- goes through ONE primitive: an in-place SUM
// all-reduce of 64-bit integers (owners contribute their bit patterns, everybody else zeros), which is exact.
struct Distributed {
    int rank = 0, world = 1;
    int (*allreduce_i64)(int64_t* buf, uint64_t n, void* user) = nullptr;  // 0 on success
    void* user = nullptr;
    bool active() const { return world > 1; }
    // the background map (by far the largest) alone on rank 0, objects round-robin over the other ranks; colocate (Config::
    // colocateBackground, BASELINE.json configs[3]: "8 object models sharded one-per-GPU"): objects round-robin over ALL ranks, the
    // background shares rank 0 with the objects that land there
    bool colocate = false;
    int owner(unsigned id) const
    {
        if (world <= 1 || id == 0) return 0;
        return colocate ? (int)((id - 1) % (unsigned)world) : 1 + (int)((id - 1) % (unsigned)(world - 1));
    }
    // Background split over the ranks (Config::shardBackground): every rank keeps a replica of the background map and takes a share of
    // its two reductions -- the surfel range it rasterises into the index map (MIN all-reduce of the z-keys) and the image rows it
    // reduces in the ICP step (SUM all-reduce of the normal-equation accumulators after every launch of the Gauss-Newton loop).
    bool shardBackground = false;
    bool ownsHere(unsigned id) const { return (id == 0 && shardBackground && active()) ? true : owner(id) == rank; }
    // for the one-owner exchanges (poses, segmentation sums): does THIS rank contribute model `id`?
    bool contributes(unsigned id) const { return (id == 0 && shardBackground && active()) ? rank == 0 : owner(id) == rank; }
    void sum(int64_t* buf, uint64_t n) const;  // throws if the collective is missing or fails
    // the same collective on a DEVICE buffer, enqueued on `stream` (RCCL): no host visit.  Optional: without it device buffers are
    // staged through the host callback.
    int (*allreduce_dev)(int64_t* dev_buf, uint64_t n, void* hip_stream, void* user) = nullptr;
    void* user_dev = nullptr;
    void sumDevice(cf_ctx* ctx, int64_t* dev_buf, uint64_t n) const;
};

class Model {
  public:
    Model(cf_ctx* ctx, unsigned char id, float confidenceThresh, bool enableFillIn, int maxSurfels,
          float maxDepth = 3.402823466e+38f, bool owned = true);
    ~Model();
    Model(const Model&) = delete;
    Model& operator=(const Model&) = delete;

    unsigned lastCount() const;
    void initialise(const uint8_t* rgba, const float* depthRaw, const float* depthFiltered, int time, float maxDepth);
    // Model::initICP (Model.cpp:350-367); frame-wide current maps are owned by `frameOdom` (model 0)
    void initICP(bool doFillIn, bool frameToFrameRGB, const float* const depthPyr[3], float depthCutoff, const uint8_t* rgba,
                 Model* frameOwner);
    // the two halves of initICP, used by the batched preparation of CoFusion::trackModels
    void trackingInputs(bool doFillIn, bool frameToFrameRGB, const float*& v, const float*& n, const uint8_t*& img) const;
    void bindFrameMaps(const float* const depthPyr[3], float depthCutoff, Model* frameOwner);
    float computeFusionWeight(float weightMultiplier) const;
    void fuse(int time, const uint8_t* rgba, const uint8_t* mask, const float* depthRaw, const float* depthFiltered, float depthCutoff,
              float weightMultiplier);
    void clean(int time, int timeDelta, float depthCutoff, const float* depthFiltered, const uint8_t* mask, float outlierCoeff);
    void predictIndices(int time, float depthCutoff, int timeDelta);
    void combinedPredict(float depthCutoff, int time, int maxTime, int timeDelta);
    void performFillIn(const uint8_t* rgba, const float* depthFiltered, bool frameToFrameRGB, bool lost);
    bool requiresFillIn(float ratio = 0.75f);
    // the same question left to the kernels that prepare the tracking (cf_odom_init_models_batch_select): device address of the counts
    // the last prefetchFillRatio() left, nullptr when this model never fills in or nothing was prefetched.  Never waits.
    const uint32_t* fillRatioDevice() const;
    void prefetchFillRatio();
    bool allowsFillIn() const { return fillIn; }
    bool fillsInHere() const { return fillIn && owned; }   // does performFillIn / prefetchFillRatio launch anything for this model?
    std::vector<float> downloadMap() const;  // count x 12 floats

    float getConfidenceThreshold() const { return confidenceThreshold; }
    void setConfidenceThreshold(float v) { confidenceThreshold = v; }
    void setMaxDepth(float d) { maxDepth = d; }
    float getMaxDepth() const { return maxDepth; }
    const Mat4f& getPose() const { return pose; }
    const Mat4f& getLastPose() const { return lastPose; }
    void overridePose(const Mat4f& p) { pose = p; lastPose = p; }
    unsigned getID() const { return id; }
    unsigned incrementUnseenCount() { if (unseenCount < 0xFFFFFFFFu) return ++unseenCount; return unseenCount; }
    void resetUnseenCount() { unseenCount = 0; }
    cf_odom* getFrameOdometry() { return odom; }
    cf_model* handle() { return model; }
    float* icpErrorSurface() { return icpError; }
    const float* vertexConfProjection() const;
    cf_track_stats lastStats{};
    bool isOwned() const { return owned; }
    // re-detection (CoFusion::setRedetection): the object's pose in the world, G * M^-1 as in the pose log, when it was deactivated ...
    Mat4f worldPoseAtDeactivation = Mat4f::identity();
    // ... and, one frame long, "reactivated in this frame": no index map, fusion or clean-up, the end-of-frame prediction only
    bool predictOnlyThisFrame = false;
    // split over the ranks (background replica): shard index / count, 0 / 1 when the model lives on one rank
    int shard = 0, shards = 1;

    struct PoseLogItem { int64_t ts; float p[7]; };  // x,y,z, qx,qy,qz,qw (Model.h:230-233)
    std::vector<PoseLogItem> poseLog;
    bool loggingPoses = false;
    bool isLoggingPoses() const { return loggingPoses; }

  private:
    friend class CoFusion;
    cf_ctx* ctx;
    cf_model* model = nullptr;
    cf_odom* odom = nullptr;
    float* icpError = nullptr;  // device f32 [H*W] (Model::icpError texture)
    Mat4f pose, lastPose;
    float confidenceThreshold;
    float maxDepth;
    unsigned id;
    unsigned unseenCount = 0;
    bool fillIn;
    bool owned = true;   // false: shadow of a model that lives on another rank (no device objects, only the replicated state)
};
typedef std::shared_ptr<Model> ModelPointer;
typedef std::list<ModelPointer> ModelList;

class Segmentation {
  public:
    Segmentation(cf_ctx* ctx, int width, int height, const Distributed* dist = nullptr);
    ~Segmentation();
    Segmentation(const Segmentation&) = delete;
    Segmentation& operator=(const Segmentation&) = delete;
    // Segmentation::performSegmentation's GT branch (Segmentation.cpp:59-119) on the host, for a frame whose label mask is a host buffer
    // (frame.mask: model-parallel runs and CF_MASKS_HOST=1); uploads the label image into fullSegmentation_dev.  Its CRF branch
    // (:124-706) is the device-resident chain below.
    SegmentationResult performSegmentationGT(ModelList& models, const FrameData& frame, unsigned char nextModelID, bool allowNew,
                                             uint8_t* fullSegmentation_dev);
    // enqueue SLIC for this frame's image ahead of enqueueCRF / collectCRF (on whatever stream the context currently uses)
    void startSlic(const uint8_t* rgba_dev);
    // ... and, behind it, everything else of the device-resident CRF chain that does not need this frame's tracking (cf_seg_early: the
    // frame's and the confidences' sums, means, depth range, average confidences, appearance features and kernel matrix).  The models'
    // confidence projections are the previous frame's prediction; enqueueCRF then finds the segmenter prepared and enqueues the rest.
    // Single-process sequences only (the confidence sums are consumed here: no collective could add the other ranks' to them).
    void startEarly(ModelList& models, const float* depth_dev, const uint8_t* rgba_dev);
    // the reference's performSegmentationCRF in two halves without a host wait in between: everything is enqueued (sums, unaries, mean
    // field, component analysis, up-sampling into fullSegmentation_dev), the decisions are collected later
    void enqueueCRF(ModelList& models, const float* depth_dev, const uint8_t* rgba_dev, unsigned char nextModelID, bool allowNew,
                    uint8_t* fullSegmentation_dev);
    SegmentationResult finishCRF();
    // ... of several sequences through shared launches (lock-step groups): collectCRF does what enqueueCRF does up to the launches and
    // describes them as a job (its arrays live in this object until the next call), runBatch enqueues the jobs of all sequences in one
    // chain (cf_seg_run_batch); finishCRF as usual.  Single-process sequences only.
    void collectCRF(ModelList& models, const float* depth_dev, const uint8_t* rgba_dev, unsigned char nextModelID, bool allowNew,
                    uint8_t* fullSegmentation_dev, cf_seg_job& job);
    static void runBatch(cf_ctx* ctx, const Segmentation& params, const std::vector<cf_seg_job>& jobs);
    // The label-mask branch (performSegmentationGT) on the device, the same trio: enqueueMasks enqueues the three kernels of
    // cf_seg_masks (label image into fullSegmentation_dev) on the context's current stream, collectMasks only describes them as a job
    // for the group's one chain (runMaskBatch), finishMasks collects the rows after the frame's host wait and enters the mask value that
    // spawned a label into gtMapping.  depth_dev is the frame's RAW depth.
    void enqueueMasks(ModelList& models, const uint8_t* mask_in_dev, const float* depth_dev, unsigned char nextModelID, bool allowNew,
                      uint8_t* fullSegmentation_dev);
    void collectMasks(ModelList& models, const uint8_t* mask_in_dev, const float* depth_dev, unsigned char nextModelID, bool allowNew,
                      uint8_t* fullSegmentation_dev, cf_seg_mask_job& job);
    static void runMaskBatch(cf_ctx* ctx, const std::vector<cf_seg_mask_job>& jobs);
    SegmentationResult finishMasks();
    // model-parallel operation: enqueueCRF put every owner's tracked pose behind the sums it all-reduces; after the frame's host wait
    // this hands out [models][18] words (pose row-major, ICP error, ICP inlier count as f32 bit patterns).  false: nothing was published
    bool fetchPublishedPoses(size_t nModels, std::vector<int64_t>& words);
    // label-mask mode under re-detection: the mask value that proposed this frame's new label is mapped to `id` instead (a reactivated
    // model keeps its old id); every value that maps to `id` is forgotten (a deactivated model: the value may propose a label again)
    void remapNewValue(unsigned char id) { if (lastNewValue > 0) gtMapping[lastNewValue & 255] = id; }
    void forgetModel(unsigned char id) { for (int v = 1; v < 256; v++) if (gtMapping[v] == id) gtMapping[v] = 0; }
    // setters (Segmentation.h:100-120); defaults are the GUI values the reference applies every frame (GUI.h:206-227)
    float unaryWeightError = 75.f, unaryKError = 0.0375f, unaryThresholdNew = 5.5f;
    float weightAppearance = 7.f, weightSmoothness = 2.f;
    float scaleFeaturesRGB = 1.0f / 10, scaleFeaturesDepth = 1.0f / 0.9f, scaleFeaturesPos = 1.0f / 1.8f;
    float minRelSizeNew = 0.015f, maxRelSizeNew = 0.4f;
    unsigned crfIterations = 10;

  private:
    SegmentationResult resultRows(const cf_seg_result& r, bool boxes) const;   // finishCRF / finishMasks
    cf_ctx* ctx;
    cf_segmenter* seg = nullptr;
    int width, height;
    uint8_t gtMapping[256];
    const Distributed* dist = nullptr;
    bool slicStarted = false;
    int pendingModels = 0;        // models of the segmentation enqueueCRF / enqueueMasks left in flight
    unsigned char pendingNextId = 0;  // the id a new label of the mask job in flight would get
    int lastNewValue = -1;            // the mask value that proposed the last frame's new label (-1: none, or the motion segmentation)
    bool posesPublished = false;  // ... which carries the owners' poses in its all-reduce
    float* zeroImage = nullptr;   // device zeros [H*W*4] standing in for the ICP error / confidence maps of shadow models
    std::vector<const float*> jobIcp, jobConf;  // collectCRF's arrays
    std::vector<uint32_t> jobIds;
  public:
    cf_seg_params deviceParams() const;   // (the group compares the sequences' settings: one batched chain per distinct set)
};

class ExportWriter;   // ExportWriter.h

class CoFusion {
  public:
    struct Config {
        int width = 640, height = 480;
        float fx = 528, fy = 528, cx = 320, cy = 240;
        int device = 0;
        int maxSurfels = 3072 * 3072;       // Model::MAX_VERTICES default (Model.cpp:92-98)
        int maxModels = 16;
        int timeDelta = 2147483647 / 2;     // openLoop (MainController.cpp:328)
        float confGlobalInit = 10.0f, confObjectInit = 0.01f;  // MainController.cpp:174-175
        float depthCutoff = 5.0f, icpWeight = 10.0f;           // GUI.h:211-212
        float outlierCoefficient = 3.0f;                       // GUI.h:213
        bool fastOdom = false, so3 = true, frameToFrameRGB = false, pyramid = true, rgbOnly = false;
        unsigned modelSpawnOffset = 22;                        // GUI.h:219
        bool enableMultipleModels = true;
        bool enablePoseLogging = false;                        // CoFusion ctor argument (CoFusion.h:59)
        int rank = 0, world = 1;                               // model-parallel operation (see Distributed)
        // Device-resident frames (FrameData::depth_dev): true = the buffers are COMPLETE when processFrame is called (e.g. a ring
        // of frames uploaded ahead); the depth filter of the new frame then runs on an auxiliary stream that is NOT ordered after
        // the work still queued on the context's stream, i.e. beside the previous frame's fusion passes.  false (default) = they
        // may be produced by work queued on that stream just before the call, and are consumed in stream order.
        bool deviceFramesComplete = false;
        // run CoFusion::predict() between tracking and fusion as the reference does (CoFusion.cpp:346).  Its outputs are overwritten by
        // the end-of-frame prediction before anything in the frame loop reads them (they are what the reference's GUI shows), so the
        // default skips the pass; results are identical either way.
        bool midFramePredict = false;
        // model-parallel operation only: split the background's index-map rasterisation (by surfel range) and ICP reduction (by image
        // rows) over all ranks, each holding a replica of the background map (see Distributed::shardBackground)
        bool shardBackground = false;
        // model-parallel operation only: object models round-robin over ALL ranks, the background sharing rank 0 with the objects that
        // land there (BASELINE.json configs[3]: 8 object models one per GPU); default: the background alone on rank 0
        bool colocateBackground = false;
        // CoFusion's `reloc` constructor argument (CoFusion.h:47, -rl on the command line): the failure detection of the frame loop --
        // a frame whose background ICP error / pose covariance is out of bounds is not fused, and after ten such frames the camera is
        // `lost`: no fusion, the clock stops (CoFusion.cpp:225, 301-338, 463, 495).  The fern-based recovery is CoFusion::setRelocalisation.
        bool reloc = false;
        // the index maps of the tracked models rasterised before the frame's host wait, with the poses on the device (framePreIndex)
        bool earlyIndexMaps = true;
        // host threads that enqueue the per-model surfel passes (fusion, clean-up, prediction) beside the calling thread, one model's
        // chain of launches each.  Pays when the host's launch rate is the limit (a profiler attached, a slow or busy host); on an idle
        // host the calling thread alone keeps the lanes fed (610 / 606 / 604 fps with 0 / 2 / 4 helpers), hence default
        // 0 = everything from the calling thread.  Results do not depend on it.
        int enqueueThreads = 0;
    };
    explicit CoFusion(const Config& cfg);
    // a sequence of a lock-step group (CoFusionGroup): the context is the group's, shared with the other sequences
    CoFusion(const Config& cfg, cf_ctx* sharedContext, int sequenceIndex);
    ~CoFusion();

    // CoFusion::processFrame (Core/CoFusion.cpp:171-524)
    bool processFrame(const FrameData& frame, const Mat4f* inPose = nullptr, float weightMultiplier = 1.f, bool bootstrap = false);
    void predict(bool lastOfFrame = false);          // CoFusion.cpp:533-545
    // CoFusion::savePly / exportPoses (CoFusion.cpp:646-783); exportDir is a prefix ("out/"); return files written or -1
    int savePly(const std::string& exportDir);
    int exportPoses(const std::string& exportDir);
    // Mesh export (Mesh.cpp over cf_mesh_*): <prefix>mesh-<id>.ply per owned active model, a triangle mesh of its
    // confident surfels extracted on the device; voxel 0: the model's mean confident radius.  Returns files written or -1.
    int saveMesh(const std::string& exportDir, float voxel = 0.f);
    // one model's mesh in the model's own frame.  index >= 0: the active models in list order (0 = background); index < 0: the kept
    // inactive model number -1 - index.  extractMesh runs both stages and keeps the result on the device (counts 0 for a model this rank
    // does not own); keptMesh: the counts of what is kept, when it is the mesh of (index, voxel) at the current tick; downloadMesh
    // copies it out.  meshTransform: Tp = globalPose * modelPose^-1, which saveMesh applies.
    void extractMesh(int index, float voxel, uint32_t* nVertices, uint32_t* nTriangles);
    bool keptMesh(int index, float voxel, uint32_t* nVertices, uint32_t* nTriangles) const;
    void downloadMesh(cf_mesh_vertex* vertices, uint32_t* triangles);
    Model* meshModel(int index);
    Mat4f meshTransform(Model& model) const;
    void setMeshMaxVoxels(uint64_t n);               // grid samples the mesher is created for (default 2^24, 64 bytes each)
    // exportSegmentation (CoFusion.cpp:235-240): when set, every segmented frame writes <prefix>Segmentation<tick>.png (8-bit labels)
    void setExportSegmentation(const std::string& prefix) { exportSegmentationPrefix = prefix; }
    // Scene rendering (Render.cpp over cf_render): every active model drawn into one view, depth-tested against the others, the
    // background in `backgroundMode`, the objects in `objectMode` (the reference's drawScene(backgroundColor, objectColor)), placed by
    // Tp = globalPose * modelPose^-1.  view == nullptr: the current camera at the frame intrinsics and size.  The view's flags / tick /
    // time_delta are replaced by `flags` and this instance's clock.  Outputs are device buffers (cf_render_output); enqueued only.
    // Single-process operation only (Distributed::active(): throws).
    void renderScene(const cf_render_view* view, int backgroundMode, int objectMode, int flags, const cf_render_output* outputs, int n);
    cf_render_view currentView() const;
    // ... into images this instance owns (valid until the next call): rgba u8x4, depth f32, labels u8 [h*w] of the view's size
    void renderSceneOwned(const cf_render_view* view, int backgroundMode, int objectMode, int flags, const uint8_t** rgba,
                          const float** depth, const uint8_t** labels, int* width, int* height);
    // after every processed frame write <prefix>Labels<n>.png (background in colour, objects in label colour), Normals<n>.png and /
    // or Viewport<n>.png (colour for all models) from the current camera, <n> the frame's number as in Segmentation<n>.png.
    // which: 1 labels | 2 normals | 4 viewport; 0 switches it off.  One rasterisation feeds all three.
    enum { ExportLabels = 1, ExportNormals = 2, ExportViewport = 4 };
    void setExportViews(const std::string& prefix, int which);
    // The per-frame exports (Segmentation<n>.png and the views) through the device PNG encoder and writer threads (ExportWriter.h,
    // DESIGN.md 4.12) instead of a read-back and zlib on the calling thread: same file names, numbering and pixels, another (valid)
    // PNG encoding.  Off by default.  The frame loop never waits for a file unless all `slots` (2..16) are busy; a failed write is
    // thrown by the next frame or by exportFlush.  workers: 1..8 writer threads.  Switching it off writes what is in flight first.
    void setExportAsync(bool on, int workers = 2, int slots = 8);
    void exportFlush();   // returns when every submitted file is closed (a no-op without setExportAsync)
    // images and bytes written, submits that found every slot busy; timing: the encoder's device events from here on (the sums are
    // those since the last call).  All zero without setExportAsync.
    void exportStats(uint64_t* images, uint64_t* bytes, uint64_t* stalls, double* deviceMs, uint64_t* deviceImages, bool timing);
    // the collective of the model-parallel mode (cfg.world > 1); must be set before the first frame
    void setAllreduce(int (*fn)(int64_t*, uint64_t, void*), void* user) { dist.allreduce_i64 = fn; dist.user = user; }
    void setAllreduceDevice(int (*fn)(int64_t*, uint64_t, void*, void*), void* user) { dist.allreduce_dev = fn; dist.user_dev = user; }
    // the library's own RCCL communicator (cf_rccl_init) as the collective of this instance: device buffers are all-reduced in place by
    // ncclAllReduce on the context's stream, host buffers through a small device staging buffer; also registers the collective of a
    // split background.  `id128` is the ncclUniqueId rank 0 created (cofusion_rccl_unique_id).  Collective call: every rank of cfg.world.
    void initRccl(const void* id128);
    // depth + colour of a frame (any device buffer) from rank `root` to every rank: ncclBroadcast on the context's stream
    void broadcast(void* dev_buf, uint64_t bytes, int root);
    int rcclSumHost(int64_t* buf, uint64_t n);  // (the host-buffer flavour of the collective; 0 on success)
    const Distributed& distributed() const { return dist; }
    ModelList& getModels() { return models; }
    ModelPointer getBackgroundModel() { return globalModel; }
    const Mat4f& getCurrPose() const { return globalModel->getPose(); }
    int getTick() const { return tick; }
    bool getLost() const { return lost; }  // CoFusion::getLost (CoFusion.h:183-185): the camera is lost (Config::reloc)
    // The recovery half of `reloc`: ElasticFusion's fern keyframe database (cf_ferns).  Off by default; with it off the
    // frame loop is what it was, launch for launch.  On: every tracked frame offers the background's fill-in maps to the database
    // (Ferns::addFrame, no host wait), a lost camera asks it for a keyframe after the end-of-frame prediction (Ferns::findFrame) and,
    // on acceptance, continues from the recovered pose (CoFusion.cpp:349-367, 321-337).  Needs Config::reloc; single process, not a
    // sequence of a lock-step group.  Calling it again replaces the database.
    void setRelocalisation(bool on, int nFerns = 500, float fernThreshold = 0.3095f, float photoThreshold = 115.0f, int minAge = 300,
                           uint64_t seed = 0, int capacity = 1024);
    void relocStats(int* keyframes, int* lastClosest, int* recoveries, int* databaseFull);
    // Global loop closure (the closeLoops branch of CoFusion.cpp:345-384, which the reference stubs; ElasticFusion's).
    // Off by default; with it off the frame loop is what it was, launch for launch.  On: a tracked frame encodes, searches and GATES its
    // fill-in maps against the database (one more launch and one host wait on a 32-byte record); a candidate runs Ferns::findFrame
    // (cf_ferns_find_frame), and an accepted one samples the deformation graph of the background map, weights the constraints the fern
    // kernel left on the device, optimises, and on acceptance moves the map and the keyframe poses, overrides the camera pose and
    // redoes the prediction.  Needs setRelocalisation on (which, called again, switches this off) and a fern count loop closure
    // accepts (CF_FERNS_MAX_SAMPLES); single process, not a sequence of a lock-step group.
    void setLoopClosure(bool on, int sampleRate = 25000);
    struct LoopStats {
        int gated = 0, candidates = 0, fernAccepts = 0;   // frames gated, candidates (match with overlap > 0.3), Ferns::findFrame accepts
        int optimised = 0, accepted = 0, failed = 0;      // graphs
        int lastKeyframe = -1, lastKeyframeTime = -1, lastNodes = 0, lastTick = -1;   // of the last fern accept: keyframe, its srcTime, graph nodes, the frame's tick
        cf_deform_result last{};
    };
    const LoopStats& loopStats() const { return loopSt; }
    // Local (model-to-model) loop closure (CoFusion.cpp:386-461, which the reference stubs; ElasticFusion's, DESIGN.md 4.14 "The local
    // half").  Off by default; with it off the frame loop is what it was, launch for launch.  On: a tracked frame in which the fern seam
    // closed no loop predicts the INACTIVE part of the background map behind the end-of-frame prediction, registers the ACTIVE
    // prediction onto it with a second tracker and runs the constraint launch, all enqueued unconditionally, then waits ONCE, on the
    // constraint launch's record, which also carries the covered-texel count.  Fewer covered texels than minInactivePixels (< 0: the
    // default, icpCountThresh; 0: the reference, no gate): nothing more.  An accepted registration samples a second, sized graph at
    // sampleRate, weights the constraints on the device, optimises in the local mode (lastDeformTime), and an accepted graph moves the
    // map with the reactivation stamp read from the depth synthesized at the estimated pose, moves the keyframe poses if there is a
    // database, overrides the camera pose and redoes the prediction.  Needs Config::timeDelta > 0 (an inactive map); single process,
    // not a sequence of a lock-step group.  Needs no fern database.
    void setLocalLoopClosure(bool on, int sampleRate = 5000, int icpCountThresh = 40000, float icpErrThresh = 5e-5f, float covThresh = 1e-5f,
                             int minInactivePixels = -1);
    struct LocalLoopStats {
        int examined = 0, skippedByGate = 0, trackerAccepts = 0;   // frames examined, stopped by the pixel gate, accept rule passed with >= 1 constraint
        int optimised = 0, accepted = 0, failed = 0;               // graphs
        int lastNodes = 0, lastConstraints = 0;                    // of the last tracker accept (constraint rows, pins included)
        int lastPinned = 0, lastTick = -1;                         // ... whether its rows carried pins, the frame's tick
        int deforms = 0, lastDeformTime = 0;
        uint32_t lastCovered = 0;                                  // covered inactive texels of the last examined frame
        cf_deform_result last{};
        cf_local_loop_record lastRecord{};                         // of the last examined frame
    };
    const LocalLoopStats& localLoopStats() const { return localSt; }
    // Relative constraints (CoFusion.cpp:373, 445-458; DESIGN.md 4.14 "Relative rows"): what makes the two closures cooperate.  Off by
    // default; with it off, or with no pair stored, every closure is what it was, launch for launch.  On: an accepted LOCAL closure
    // leaves a few of its constraints behind as pairs (moved source, target, their times) in a device ring of 128 on the global graph
    // (cf_deform_pick_relative, no host round trip), and every later GLOBAL closure -- the fern seam's and deformBackground's -- takes
    // the stored pairs as rows 10 (phi(src) - phi(tgt)), so that it cannot pull apart what a local closure registered.  Switching it
    // off keeps the allocation and empties the store.  Single process, not a sequence of a lock-step group.
    void setRelativeConstraints(bool on);
    // caller-supplied pairs, appended to the store as deformBackground takes caller-supplied constraints (host arrays [n][3], [n])
    void addRelativeConstraints(const float* src, const float* dst, const float* srcTime, const float* dstTime, int n);
    // the stored pairs in store order: out [capacity][8] (source xyz, srcTime, target xyz, dstTime); returns how many the store holds
    int relativeConstraints(float* out, int capacity);
    struct RelativeStats { long long appended = 0; long long overwritten = 0; int stored = 0; int usedByLastClosure = 0; int lastPicked = 0; };
    RelativeStats relativeStats();
    // test access: what the last accepted local closure worked on, readable until the next frame is processed -- its constraint rows
    // (src, dst [rows][3], time [rows]; pinned: rows 2 k and 2 k + 1), the old time of every constraint (targetTime [rows or rows / 2]),
    // the last_deform_time its graph was optimised with, and that graph (nodes [n][4], accepted params [n][12]).  Outputs nullable;
    // rowCapacity / nodeCapacity: what the arrays hold.  Returns false when no local closure has been accepted.
    bool localClosureDownload(int* rows, int* pinned, int* lastDeformTime, float* src, float* dst, float* time, float* targetTime, int rowCapacity,
                              int* nodes, float* nodePos, float* params, int nodeCapacity);
    bool isGroupSequence() const { return !ownsCtx; }
    // Loop closure of the background map from caller-supplied constraints: sample the deformation graph, weight the
    // constraint points, optimise, and on acceptance move the map (cf_deform_*) and redo the prediction.  Returns the node count.
    int deformBackground(const float* src, const float* dst, const float* srcTime, const float* dstTime, int n, bool pin, int sampleRate,
                         cf_deform_result* result);
    // Re-detection of inactive models (the reference's redetectModels is empty, CoFusion.cpp:599-602).  Off by default;
    // with it off the frame loop is what it was.  On: a frame whose segmentation reports a new label scores the most recent
    // `maxCandidates` (1..16) inactive models against the frame (cf_redetect_score), each at the pose it would have now had it not
    // moved in the world since it was deactivated, BEFORE a model is spawned.  fit = agree_on_label / (agree + seen_through) >= minFit
    // and cover = covered / label_pixels >= minCover make a candidate eligible; the one with the largest agree_on_label (ties: the
    // earlier in the list) is reactivated with its old id, map, confidence threshold and pose log instead of a spawn.  One more host
    // wait in such a frame.  keepMinSurfels / keepConfThreshold: the rule by which a deactivated model is kept at all (4000 / 0.3).
    // Single process only (throws for a model-parallel instance); works for a sequence of a lock-step group.
    void setRedetection(bool on, float minFit = 0.5f, float minCover = 0.044f, float depthTol = 0.10f, int maxCandidates = 8,
                        unsigned keepMinSurfels = 4000, float keepConfThreshold = 0.3f);
    struct RedetectCandidate { unsigned id; cf_redetect_counts counts; float fit, cover; bool eligible; };
    struct RedetectStats { int attempts = 0, reactivations = 0, lastId = -1; };
    const RedetectStats& redetectStats() const { return redetectSt; }
    // the candidates of the last attempt in list order, the number of pixels its new label had, the position of the winner (-1: none)
    const std::vector<RedetectCandidate>& redetectLast(uint32_t* labelPixels = nullptr, int* winner = nullptr) const
    {
        if (labelPixels) *labelPixels = redetectLabelPixels;
        if (winner) *winner = redetectWinner;
        return redetectCands;
    }
    // The search behind it (DESIGN.md 4.13 "Search"), for an object that came back SOMEWHERE ELSE.  Needs setRedetection on; off by
    // default, and with it off every frame is what it was.  Runs only in a frame whose static pass found nobody eligible: candidates
    // whose colour histogram intersects the label's by at least `minColour` are ranked by that similarity; the first `maxRegistered`
    // are registered onto the label's pixels (cf_redetect_register, at most `iterations` steps and host waits each), re-scored at the
    // registered pose and judged by minFit / minCover as above; the winner is reactivated at the registered pose.  Envelope: any
    // translation that keeps the object in view, turns up to about 10 degrees (degrading towards 20).  Single process only.
    void setRedetectionSearch(bool on, int iterations = 10, float minColour = kRedetectMinColour, int maxRegistered = 2);
    static constexpr float kRedetectMinColour = 0.175f;   // between the weakest returning object (0.67) and the strongest stranger (0.046) of the facade scenes, DESIGN.md 4.13
    struct RedetectSearchCandidate {
        unsigned id = 0; float colour = 0.f; bool registered = false, converged = false; int iterations = 0;
        uint32_t firstInliers = 0, lastInliers = 0; float rms = 0.f, moved = 0.f;   // moved: front-facing centroid, registered against static pose (m)
        cf_redetect_counts counts{}; float fit = 0.f, cover = 0.f; bool eligible = false;   // the score at the registered pose
    };
    // the candidates of the last attempt's search in the order of redetectLast (empty when that attempt did not search), the winner's
    // position (-1: none), and the number of frames that searched
    const std::vector<RedetectSearchCandidate>& redetectSearchLast(int* winner = nullptr, int* attempts = nullptr) const
    {
        if (winner) *winner = searchWinner;
        if (attempts) *attempts = searchAttempts;
        return searchCands;
    }
    size_t numInactiveModels() const { return inactiveModels.size(); }
    // The motion-CRF chain's tracking-independent half beside the tracking launches (Segmentation::startEarly).  On by default; off
    // leaves the whole chain behind the tracker -- the same results bit for bit, for A/B measurements and parity tests.
    void setSegEarly(bool on) { segEarly = on; }
    const uint8_t* maskDevice() const { return mask_dev; }
    Segmentation& segmentation() { return *labelGenerator; }
    cf_ctx* context() { return ctx; }
    Config cfg;

    // ---- the stages of processFrame (see CoFusion.cpp); CoFusionGroup runs them stage by stage over its sequences ----
    struct TrackBatch {   // the trackers of one set of lock-step launches: the owned models of one frame, or of several sequences' frames
        struct Item { Model* model; Model* owner; const float* depthPyr[3]; const uint8_t* frameRgba; float maxDepth;
                      const float* predV; const float* predN; const uint8_t* predImg;
                      // the fill-in flavour of the three and the device counts that decide between them (fillCounts == nullptr: no choice)
                      const float* altV; const float* altN; const uint8_t* altImg; const uint32_t* fillCounts; };
        std::vector<Item> items;
    };
    void frameBegin(const FrameData& frame, const Mat4f* inPose, float weightMultiplier, bool bootstrap);
    bool frameTracks() const { return st.willTrack; }
    void trackCollect(TrackBatch& batch) { trackCollect(batch, st.pyr); }
    static void trackLaunch(cf_ctx* ctx, TrackBatch& batch, const Config& cfg);
    // segmentation enqueued (jobs != nullptr: described as a job for the group's shared launches instead -- Segmentation::runBatch)
    void frameSegment(std::vector<cf_seg_job>* jobs, std::vector<cf_seg_mask_job>* maskJobs);
    void framePreIndex();
    void frameCollect();           // the frame's host wait (poses + segmentation decisions), model bookkeeping
    void frameFuse(bool join, int laneOffset);
    // ... in two halves for a lock-step group: every sequence adds its models' passes to ONE batch (cf_models_frame_passes), the group
    // launches it, each sequence then runs its fill-in
    bool passesBatched() const { return !dist.active(); }
    float depthLimit() const { return maxDepthProcessed; }
    void frameFuseCollect(std::vector<cf_model_pass>& items);
    void frameFuseFinish();
    void frameEnd();

  private:
    struct FrameStage {   // what the stages of one frame hand to each other
        const FrameData* frame = nullptr; const Mat4f* inPose = nullptr; float weightMultiplier = 1.f; bool bootstrap = false;
        unsigned b = 0; bool willTrack = false, slicAside = false, fuseNow = false, allowNew = false, segOnDevice = false;
        bool masksAside = false, masksOnDevice = false;   // the mask chain: lane 7 forked at frameBegin; enqueued by frameSegment
        const uint8_t* maskIn = nullptr;                  // the frame's label mask in device memory (given so, or uploaded from the host)
        const float* pyr[3] = {nullptr, nullptr, nullptr};
    } st;
    bool ownsCtx = true;
    bool segEarly = true;
    int markBase = 0;   // this sequence's four event slots of the context (cf_mark)
    void trackCollect(TrackBatch& batch, const float* const depthPyr[3]);
    void spawnObjectModel();
    // CoFusion::redetectModels (the name the reference left empty): scores the candidates against the current frame, whose label image
    // holds `newLabel`; returns the accepted model, taken out of inactiveModels with its hypothesis pose set, or null
    ModelPointer redetectModels(unsigned char newLabel);
    struct { bool on = false; float minFit = 0.5f, minCover = 0.044f, depthTol = 0.10f; int maxCandidates = 8; } redetect;
    RedetectStats redetectSt;
    std::vector<RedetectCandidate> redetectCands;
    uint32_t redetectLabelPixels = 0;
    int redetectWinner = -1;
    int searchModels(const std::vector<cf_redetect_candidate>& in, std::vector<Mat4f>& hyp, const cf_redetect_frame& f);
    struct { bool on = false; int iterations = 10; float minColour = kRedetectMinColour; int maxRegistered = 2; } search;
    std::vector<RedetectSearchCandidate> searchCands;
    int searchWinner = -1, searchAttempts = 0;
    void moveNewModelToList();
    ModelList::iterator inactivateModel(ModelList::iterator it);
    unsigned char getNextModelID(bool assign = false);
    void trackModels(const float* const depthPyr[3]);   // enqueues; poses arrive with fetchTracking
    void fetchTracking(bool exchange);
    void exchangeTracking();
    std::vector<Model*> trackPending;
    Distributed dist;

    cf_ctx* ctx = nullptr;
    ModelList models, inactiveModels;
    ModelPointer newModel, globalModel;
    unsigned char nextID = 0;
    std::unique_ptr<Segmentation> labelGenerator;
    int tick = 1;
    float maxDepthProcessed = 20.0f;
    unsigned spawnOffset = 0;
    int64_t* rcclStage = nullptr;      // device staging buffer of the host-buffer all-reduce (initRccl)
    uint64_t rcclStageWords = 0;
    bool capReported = false;  // the model cap suppressed a spawn and said so
    bool lost = false;          // CoFusion.h:362 (reloc)
    int trackingCount = 0;      // CoFusion.h:364
    cf_ferns* ferns = nullptr;  // setRelocalisation
    float fernThreshold = 0.3095f;
    int fernMinAge = 300, fernLastClosest = -1, recoveries = 0;
    bool lastFrameRecovery = false;   // CoFusion.h:363
    void fernsAfterPredict();
    cf_deform* deform = nullptr;   // deformBackground, setLoopClosure (created at first use)
    bool closeLoops = false;       // setLoopClosure
    int loopSampleRate = 25000, fernCount = 0, fernFirstAdd = -1;   // fernFirstAdd: tick of the first frame offered to the database
    LoopStats loopSt;
    bool closeLoop(const cf_ferns_gate& gate);
    // the body deformBackground and closeLoop share: sample, weigh (the caller's upload), optimise, and on acceptance the map pass with
    // the reactivation stamp (at *correctedPose when given, which becomes the camera pose), the keyframe poses and the prediction
    // graph: the object that is sampled; lastDeformTime < 0: the global mode (cf_deform_optimise), >= 0: the local mode, whose stamp reads
    // the depth synthesized from the un-deformed map at the corrected pose instead of the frame's
    int deformMap(cf_deform* graph, int sampleRate, const std::function<int()>& weigh, int clockAhead, const Mat4f* correctedPose, int keyframes,
                  int lastDeformTime, cf_deform_result* result);
    // setLocalLoopClosure
    bool closeLocalLoops = false;
    int localSampleRate = 5000, localMinInactive = 40000;
    cf_local_loop_thresholds localTh{1e-5f, 40000, 5e-5f};
    cf_local_loop* localLoop = nullptr;
    cf_deform* localDeform = nullptr;    // the sized graph (CF_DEFORM_MAX_CONSTRAINTS_SIZED)
    cf_odom* modelToModel = nullptr;     // CoFusion::modelToModel
    float* localDepth = nullptr;         // device f32 [H * W]: the synthesized depth of an accepted closure
    LocalLoopStats localSt;
    bool fernClosedThisFrame = false;
    void localLoopAfterPredict();
    bool relativeOn = false;        // setRelativeConstraints
    int relLastPicked = 0;
    int localClosureLdt = 0, localClosureRows = 0, localClosurePinned = 0;   // of the last accepted local closure (localClosureDownload)
    void releaseLocalLoop();
    // device frame buffers (CoFusion::textures)
    // filtered depth + its pyramid are double buffered: the filter of frame t+1 runs on an auxiliary stream while the fusion
    // passes of frame t still read frame t's filtered depth (processFrame)
    float *depth_dev = nullptr, *depthFiltered_dev = nullptr, *depthPyr1 = nullptr, *depthPyr2 = nullptr;
    float *depthFilteredBuf[2] = {nullptr, nullptr}, *depthPyr1Buf[2] = {nullptr, nullptr}, *depthPyr2Buf[2] = {nullptr, nullptr};
    unsigned frameParity = 0;
    uint8_t *rgba_dev = nullptr, *rgb_dev = nullptr, *mask_dev = nullptr;
    uint8_t* stage[2] = {nullptr, nullptr};   // pinned staging of the host-input path (depth f32 | rgb u8x3 | mask u8)
    uint8_t* maskIn_dev = nullptr;            // where a host label mask is uploaded to (hostMasksOnDevice)
    bool hostMasksOnDevice = false;           // host masks take the mask kernels (world == 1) instead of the host loops
    unsigned uploads = 0;
    const float* curDepth = nullptr;   // device pointers of the frame being processed
    const uint8_t* curRgba = nullptr;
    unsigned modelKeepMinSurfels = 4000;
    float modelKeepConfThreshold = 0.3f;
    bool enableSmartModelDelete = true;
    std::string exportSegmentationPrefix;
    // scene rendering: created at first use, grown when a larger view is asked for (Render.cpp)
    cf_renderer* renderer = nullptr;
    int renderW = 0, renderH = 0;
    uint8_t* renderImages = nullptr;   // device: 3 RGBA images | depth f32 | labels u8, each of renderW x renderH
    std::string exportViewsPrefix;
    int exportViewsWhich = 0;
    void ensureRenderer(int w, int h);
    void releaseRenderer();
    void exportViews(int frameTick);
    std::unique_ptr<ExportWriter> exportWriter;   // setExportAsync
    // mesh export: created at first use (Mesh.cpp)
    cf_mesher* mesher = nullptr;
    uint64_t meshMaxVoxels = 1ull << 24;
    bool meshKept = false; int meshIndex = 0; float meshVoxel = 0.f; int meshTick = 0; uint32_t meshVertices = 0, meshTriangles = 0;
    void releaseMesher();
    bool useLanes = true;  // per-model auxiliary streams
    std::shared_ptr<EnqueuePool> pool;                      // Config::enqueueThreads helpers
    void modelPasses(Model& model, bool fuse, float weightMultiplier, bool lost);
    void fuseAndPredict(bool fuse, float weightMultiplier, bool lost, bool join = true, int laneOffset = 0);
};

// Several independent sequences on one GPU in lock-step: one context, one set of tracking launches for the trackers of all of them
// (CoFusion.cpp, "CoFusionGroup").  Same configuration (image size, intrinsics, options) for every sequence.
class CoFusionGroup {
  public:
    CoFusionGroup(const CoFusion::Config& cfg, int sequences);
    ~CoFusionGroup();
    CoFusionGroup(const CoFusionGroup&) = delete;
    CoFusionGroup& operator=(const CoFusionGroup&) = delete;
    int size() const { return (int)seqs.size(); }
    CoFusion& sequence(int s) { return *seqs.at((size_t)s); }
    // one frame of EVERY sequence: frames[s] goes to sequence s (inPoses: nullable, entries nullable)
    void processFrames(const FrameData* frames, const Mat4f* const* inPoses = nullptr);
    cf_ctx* context() { return ctx; }
    bool hasFailed() const { return failed; }

  private:
    void stepAll(const FrameData* frames, const Mat4f* const* inPoses);
    CoFusion::Config cfg;
    cf_ctx* ctx = nullptr;
    std::vector<std::unique_ptr<CoFusion>> seqs;
    bool failed = false;  // a stage threw: the sequences are out of step, further frames are refused
};

}  // namespace cofusion
