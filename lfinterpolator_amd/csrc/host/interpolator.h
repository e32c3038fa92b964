// interpolator.h — host orchestration of the light-field interpolation.  The public surface is source-compatible with
// the reference's Interpolator (reference src/interpolator.h:5-37): same constructor, destructor and interpolate()
// signature, same method strings ("STD", "TEN_WM"), same exceptions.  All device work goes through the C-ABI of
// include/lfi.h; this file includes no HIP header.
#pragma once

#include <array>
#include <memory>
#include <string>
#include <vector>

#include "../../../include/lfi.h"
#include "lenticular.h"
#include "params.h"
#include "vec.h"
#include <fstream>

#include "y4m.h"

class LfLoader;

class Interpolator
{
    public:
        // inChromaSite: how the chroma of a light-field video's frames is sited — lfi::Y4M_SITE_CENTRE, _LEFT or _AUTO (by the files' C tag:
        // C420mpeg2 left, everything else centre; the cameras' tags must agree then)
        Interpolator(std::string inputPath, int inChromaSite = lfi::Y4M_SITE_CENTRE);
        // A mosaic as input: inputPath is ONE file that holds every image as a tile of a frame of tiles.x × tiles.y tiles — an image (PNG,
        // JPEG, PPM: lfi_upload_mosaic) or a .y4m whose every frame is such a frame (lfi_upload_mosaic_yuv; a light-field video: frame t is
        // time step t, isVideo() is true).  rowsOrder false: the tiles are the cameras of a tiles.x × tiles.y grid (LFI_MOSAIC_GRID);
        // true: they are the images of a (tiles.x·tiles.y) × 1 grid in reading order (LFI_MOSAIC_ROWS: a quilt); bottomUp: the tile rows
        // count from the frame's bottom (Looking-Glass quilts).  The image size is the frame's divided by the tiles: a remainder throws,
        // and so do an odd quotient and C420p10 for a .y4m — before any GPU is touched
        struct MosaicInput
        {
            lfi::IVec2 tiles{0, 0};
            bool rowsOrder{false}, bottomUp{false};
        };
        Interpolator(std::string inputPath, int inChromaSite, MosaicInput mosaic);
        ~Interpolator();
        void interpolate(std::string outputPath, std::string trajectory, float focus, float range, std::string method, float effect, float aspect);

        // additions (defaults keep the reference's behaviour)
        void setViewCount(int count) { viewCount = count; }                // reference: always 64 (src/kernels.cu:11-13)
        void setBenchmarkRuns(size_t runs) { kernelBenchmarkRuns = runs; } // reference: 100 (src/interpolator.h:13)
        static void setDefaultDevice(int index) { defaultDevice = index; } // GPU used by Interpolator(path)
        // all-focus TEN_WM reads the filtered map 1 like STD instead of the reference's map 0 (src/kernels.cu:430 vs :326)
        void setUnifiedFocusMap(bool on) { unifiedFocusMap = on; }
        // also write quilt.png: the views as one image of cols × rows tiles (what scripts/viewsToQuilt.sh montages, 5×9 there)
        void setQuilt(lfi::IVec2 tiles) { quiltTiles = tiles; }
        // … with every view resized to a tile of width × height pixels on the device first (lfi_download_quilt_tiles_scaled: an exact area
        // filter, at most the views' size) — montage's -geometry; needs setQuilt
        void setQuiltTile(lfi::IVec2 size) { quiltTile = size; }
        // also write native.png: the native image of a lenticular display of width × height pixels whose lens sheet the calibration
        // describes (lenticular.h), interlaced on the device from the first `views` views (0: all of them), each resized to a tile of
        // tile.x × tile.y pixels first (0: the views' size, read in place) — lfi_download_native.  One GPU: every view in one context
        // flags: LFI_LENT_BGR, LFI_LENT_BILINEAR, LFI_LENT_BLEND — the filtered native image (include/lfi.h)
        void setNative(lfi::IVec2 size, lfi::LensCalibration lens, lfi::IVec2 tile = {0, 0}, int views = 0, uint32_t flags = 0)
        {
            nativeFlags = flags;
            nativeSize = size;
            nativeLens = lens;
            nativeTile = tile;
            nativeViews = views;
        }
        // also write the views as the frames of one Y4M video file, in view order: 8-bit YUV 4:2:0 converted on the device
        // (lfi_download_views_yuv420; matrix: LFI_YUV_BT709 / _BT601, range: LFI_YUV_LIMITED / _FULL) at fpsNum / fpsDen frames per second; with
        // several GPUs every one converts and downloads its own views into its part of one host buffer
        void setY4m(std::string path, int fpsNum = 30, int fpsDen = 1, int matrix = LFI_YUV_BT709, int range = LFI_YUV_LIMITED)
        {
            y4mPath = path;
            y4mFps = {fpsNum, fpsDen};
            yuvMatrix = matrix;
            yuvRange = range;
        }
        // also write the views as raw NV12 frames (the Y plane, then interleaved Cb/Cr; tightly packed) into one file, in view order:
        // converted on the device into the tight NV12 layout (lfi_download_views_yuv), same matrix, range and rate as setY4m — the two may
        // be combined and share them.  The file stays open over the time steps like the Y4M file; opening it prints the ffmpeg options
        void setNv12(std::string path, int fpsNum = 30, int fpsDen = 1, int matrix = LFI_YUV_BT709, int range = LFI_YUV_LIMITED)
        {
            nv12Path = path;
            y4mFps = {fpsNum, fpsDen};
            yuvMatrix = matrix;
            yuvRange = range;
        }
        // also write the views as raw P010 frames (NV12's layout with 16-bit samples, the 10-bit code in the upper bits; tightly packed) into
        // one file, in view order: converted on the device into the tight P010 layout (lfi_download_views_yuv with LFI_YUV_P010), same
        // matrix, range and rate as setY4m; may be combined with the others.  Opening the file prints the ffmpeg options
        void setP010(std::string path, int fpsNum = 30, int fpsDen = 1, int matrix = LFI_YUV_BT709, int range = LFI_YUV_LIMITED)
        {
            p010Path = path;
            y4mFps = {fpsNum, fpsDen};
            yuvMatrix = matrix;
            yuvRange = range;
        }
        // the bits per sample of the frames setY4m and setQuiltY4m write: 8, or 10 — I010 samples (lfi_download_views_yuv /
        // lfi_download_quilt_yuv with LFI_YUV_I010) under the tag C420p10, which carries no siting: opening the file prints the siting in use
        // and the ffmpeg option that states it.  setRgbdY4m refuses 10
        void setYuvDepth(int depth) { yuvDepth = depth; }
        // deep views (LFI_FLAG_DEEP_VIEWS): fixed-focus renders keep 10 bits per channel on the device; the 10-bit video outputs (--p010,
        // --y4m at 10 bits) are then converted from them (LFI_YUV_DEEP), and setGbrp10 stores them as raw gbrp10le planes
        void setDeep(bool on) { deep = on; }
        void setGbrp10(std::string path) { gbrp10Path = path; }
        // in-frame edges (LFI_FLAG_IN_FRAME): fixed-focus renders leave out the samples that fall outside their image and scale the rest back to
        // the full weight, instead of clamping them to the image's edge; every output is then made of those views by the same calls
        void setInFrame(bool on) { inFrame = on; }
        // linear-light blending (LFI_FLAG_LINEAR_LIGHT): fixed-focus renders decode every sample from sRGB to linear light before the weighted
        // sum and encode the sum; every output is then made of those views by the same calls
        void setLinearLight(bool on) { linearLight = on; }
        // 10 where the input is a light-field video whose files say C420p10 (they are uploaded as I010 frames: lfi_upload_images_yuv), else 8
        int inputDepth() const;
        // also write the quilt of setQuilt (scaled by setQuiltTile) as ONE frame of a Y4M video file: resized and converted to 8-bit YUV 4:2:0
        // on the device (lfi_download_quilt_yuv into a host I420 frame; even tile sizes take one kernel and no RGBA quilt), same matrix, range
        // and rate as setY4m.  The file stays open over the time steps: a light-field video gives a quilt video, one frame per step.  One GPU
        void setQuiltY4m(std::string path, int fpsNum = 30, int fpsDen = 1, int matrix = LFI_YUV_BT709, int range = LFI_YUV_LIMITED)
        {
            quiltY4mPath = path;
            y4mFps = {fpsNum, fpsDen};
            yuvMatrix = matrix;
            yuvRange = range;
        }
        // also write ONE view with a focus map beside it as one frame of a Y4M video file, 2·tile.x × tile.y: RGB-D, the colour left, the depth right
        // (lfi_download_rgbd_yuv into a host I420 frame: one kernel resizes and converts both halves).  view: −1 = the middle one (views / 2);
        // tile: {0, 0} = the views' size, else even and at most it; map: 0 as estimated, 1 filtered; invert: 255 − the map's value.  With
        // setViewMaps the view's own map is stored.  Needs an all-focus render (range > 0) and one GPU; same matrix, range and rate as setY4m.
        // The file stays open over the time steps: a light-field video gives an RGB-D video, one frame per step
        void setRgbdY4m(std::string path, int view = -1, lfi::IVec2 tile = {0, 0}, int map = 1, bool invert = false, int fpsNum = 30, int fpsDen = 1,
                        int matrix = LFI_YUV_BT709, int range = LFI_YUV_LIMITED)
        {
            rgbdY4mPath = path;
            rgbdView = view;
            rgbdTile = tile;
            rgbdMap = map;
            rgbdInvert = invert;
            y4mFps = {fpsNum, fpsDen};
            yuvMatrix = matrix;
            yuvRange = range;
        }
        // a light-field video as input (a directory of <row>_<col>.y4m files, one per camera): its frames go to the device as they are, 1.5
        // bytes per pixel from page-locked memory, and become the RGBA images there (one lfi_upload_images_yuv420 call for the grid).
        // interpolate() renders time step setInputFrame(t), 0 by default, t in [0, frameCount()); called again after another setInputFrame
        // it uploads that step and renders it with everything else unchanged — and appends its views to the ONE video file of setY4m.
        // matrix: LFI_YUV_BT709 / _BT601; range: LFI_YUV_LIMITED / _FULL, or -1 for the files' XCOLORRANGE tag (none: limited); chroma:
        // LFI_CHROMA_BILINEAR / _NEAREST
        bool isVideo() const;
        int frameCount() const; // 1 for image inputs
        void setInputFrame(int t);
        void setInputYuv(int matrix, int range, int chroma)
        {
            inMatrix = matrix;
            inRange = range;
            inChroma = chroma;
            loadedFrame = -1;
        }
        // a light-field video rendered at fixed focus on one GPU: after the first time step's parameters are set the context keeps only the
        // derived planar copy of the inputs (lfi_release_inputs), and every later step's frames go straight into it
        // (lfi_upload_images_yuv_derived) — less than half the device memory, one pass per step.  The files written are the same
        void setLeanInputs(bool on) { leanInputs = on; }
        // the chroma siting of the frames written by setY4m, setNv12 and setQuiltY4m (lfi_set_yuv_siting's out_siting): LFI_YUV_SITING_CENTRE
        // (Y4M files say C420jpeg) or _LEFT (MPEG-2 / H.264 siting: C420mpeg2; what an encoder assumes of untagged NV12).  setRgbdY4m
        // refuses left
        void setChromaSite(int siting) { outSiting = siting; }
        // closes the video files of setY4m, setNv12, setQuiltY4m and setRgbdY4m (interpolate() leaves them open for the next time step's views); throws when that fails
        void finish();
        float lastAverageTime() const { return averageTime; }
        // render on GPUs 0 … count-1 of this node: views are split into contiguous ranges, the grid is broadcast once (RCCL)
        void setGpuCount(int count) { gpuCount = count; }
        // a focus per view: view i is rendered at focus + ((end − focus) / (views − 1))·i (a focus pull; with a single-point trajectory a
        // focal stack) through lfi_set_view_offsets — fixed-focus renders only
        void setFocusEnd(float end) { focusEnd = end; perViewFocus = true; }
        // each view's shifts taken from its own camera position instead of the trajectory's centre (the reference's only choice): integer
        // rows through lfi_set_view_offsets for fixed focus (with setFocusEnd: at each view's focus), float rows through
        // lfi_set_view_float_offsets for all-focus renders
        void setViewCentred(bool on) { viewCentred = on; }
        // with setViewCentred and all-focus rendering: every view's focus map estimated at its own camera (lfi_view_focus_maps) instead of
        // one at the trajectory's centre; the maps are stored per view (map0_NN.png, map1_NN.png)
        void setViewMaps(bool on) { viewMaps = on; }
        // autofocus: interpolate()'s focus and range give the SEARCH interval [focus, focus + range] (range > 0); the focus curve of the
        // region {x0, y0, x1, y1} (all zero: the whole frame) is taken over `steps` candidates on the first GPU (lfi_focus_curve) and the
        // views are rendered at its minimum as a fixed-focus render.  Not with setFocusEnd, setViewCentred, setViewMaps.
        // stepsGiven (the caller chose `steps`, it is not a default): the whole frame over a multiple of 32 candidates up to 256 is taken as
        // the one tile of lfi_focus_tiles_steps(1, 1, steps) — by definition the same focus and index, from the factored estimate
        void setAutofocus(std::array<int, 4> region, int steps, bool stepsGiven = false)
        {
            autofocus = true;
            autofocusRegion = region;
            autofocusSteps = steps;
            autofocusStepsGiven = stepsGiven;
        }
        float lastAutofocus() const { return focus; }
        // focus tiles: before anything is rendered, the focus curve's minimum of every tile of a columns × rows grid over the frame
        // (lfi_focus_tiles on the first GPU, over [focus, focus + range], range > 0) is printed, one line per tile
        void setFocusTiles(lfi::IVec2 grid) { focusTiles = grid; }
        // auto range, for all-focus renders: the tiles' minima over [focus, focus + range] give the interval the map is then estimated over
        // and the views rendered with (lfi::focusAutoRange) instead of the interval given.  Not with setAutofocus
        void setAutoRange(lfi::IVec2 grid) { autoRange = grid; }
        // the candidates the focus tiles of setFocusTiles / setAutoRange choose from: a multiple of 32 up to 256 (lfi_focus_tiles_steps)
        void setTileSteps(int steps) { tileSteps = steps; }
        // the candidates the focus map (one map at the trajectory's centre) chooses from: a multiple of 32 up to 256 (lfi_set_focus_steps);
        // per-view maps, the focus tiles (setTileSteps) and autofocus keep their own numbers
        void setMapSteps(int steps) { mapSteps = steps; }
        // after the render, compare every view with NN.png of this directory (the names storeResults writes; the reference's
        // scripts/compareDirs.sh) in one lfi_compare_views call and print "compare NN psnr … ssim … maxdiff … differing …" per view, then
        // "compare all psnr … ssim …".  One GPU
        void setCompareDir(std::string dir) { compareDir = dir; }
        // render the views with the OTHER method first (same parameters, focus mode, layout, per-view settings), keep them on the device
        // (lfi_keep_views), render with the method asked for and compare against the kept views there; the same lines.  One GPU
        void setCompareMethods(bool on) { compareMethods = on; }

        // synthetic cols×rows grid of width×height images instead of a directory
        Interpolator(lfi::IVec2 colsRows, lfi::IVec2 resolution, uint32_t seed, int device = 0);

    private:
        size_t kernelBenchmarkRuns{100};
        int viewCount{LFI_REFERENCE_VIEWS};
        static int defaultDevice;
        int device{defaultDevice};
        bool unifiedFocusMap{false};
        lfi::IVec2 quiltTiles{0, 0};
        lfi::IVec2 quiltTile{0, 0}; // 0: the views' size, unscaled
        lfi::IVec2 nativeSize{0, 0}; // 0: no native image
        lfi::LensCalibration nativeLens;
        lfi::IVec2 nativeTile{0, 0}; // 0: the views' size, read in place
        int nativeViews{0};          // 0: all views
        uint32_t nativeFlags{0};     // LFI_LENT_BGR | LFI_LENT_BILINEAR | LFI_LENT_BLEND
        std::string y4mPath;         // empty: no video file
        lfi::IVec2 y4mFps{30, 1};
        int yuvMatrix{LFI_YUV_BT709};
        int yuvRange{LFI_YUV_LIMITED};
        std::unique_ptr<lfi::Y4mWriter> y4mWriter; // open from the first stored step to finish()
        std::string nv12Path;                      // empty: no raw NV12 file
        std::string p010Path;                      // empty: no raw P010 file
        std::ofstream p010File;                    // open from the first stored step to finish()
        int yuvDepth{8};                           // setYuvDepth
        bool deep{false};                          // setDeep
        bool inFrame{false};                       // setInFrame
        bool linearLight{false};                   // setLinearLight
        std::string gbrp10Path;                    // empty: no raw gbrp10le file
        std::ofstream gbrp10File;                  // open from the first stored step to finish()
        std::string quiltY4mPath;                  // empty: no quilt video
        std::unique_ptr<lfi::Y4mWriter> quiltY4mWriter; // open from the first stored step to finish()
        std::string rgbdY4mPath;                   // empty: no RGB-D video
        int rgbdView{-1}, rgbdMap{1};              // -1: the middle view
        lfi::IVec2 rgbdTile{0, 0};                 // 0: the views' size
        bool rgbdInvert{false};
        std::unique_ptr<lfi::Y4mWriter> rgbdY4mWriter; // open from the first stored step to finish()
        std::ofstream nv12File;                    // open from the first stored step to finish()
        std::unique_ptr<LfLoader> video;           // the input, where it is a light-field video
        MosaicInput mosaicInput;                   // tiles.x > 0: the input is a mosaic file
        std::unique_ptr<lfi::Y4mReader> mosaicVideo; // the input, where it is a Y4M mosaic: a light-field video in one file
        lfi_mosaic mosaicMap() const;
        void loadMosaic();
        void uploadMosaicFrame();
        int inputFrame{0}, loadedFrame{-1};        // the time step to render / the one on the device
        int inMatrix{LFI_YUV_BT709}, inRange{-1}, inChroma{LFI_CHROMA_BILINEAR};
        int inSiteMode{lfi::Y4M_SITE_CENTRE}; // the constructor's inChromaSite
        int inSiting{LFI_YUV_SITING_CENTRE};  // what it resolves to for the videos that were opened
        int outSiting{LFI_YUV_SITING_CENTRE}; // setChromaSite
        bool leanInputs{false}, inputsReleased{false}; // setLeanInputs / lfi_release_inputs has been called on the context
        uint8_t *inFrames{nullptr};                // one I420 frame per camera, page-locked where that works
        bool inFramesPinned{false};
        std::vector<uint8_t> inFramesPageable;
        lfi_ctx *context{nullptr};
        int gpuCount{1};
        bool perViewFocus{false};
        bool viewCentred{false};
        bool viewMaps{false};
        float focusEnd{0};
        bool autofocus{false};
        std::array<int, 4> autofocusRegion{0, 0, 0, 0}; // x0, y0, x1, y1
        int autofocusSteps{32};
        bool autofocusStepsGiven{false};
        int tileSteps{32};
        lfi::IVec2 focusTiles{0, 0}; // 0: off
        lfi::IVec2 autoRange{0, 0};  // 0: off
        int mapSteps{32};
        std::string compareDir;      // empty: off
        bool compareMethods{false};
        std::vector<lfi_ctx *> contexts; // one per GPU; contexts[0] == context
        std::vector<int> viewStart;      // first view of each GPU's range (size gpuCount + 1)
        float focus{0};
        float range{0};
        float averageTime{0};
        size_t channels{4};
        lfi::IVec2 colsRows;
        lfi::IVec3 resolution;
        std::string input;
        void init();
        void loadGPUData();
        void uploadVideoFrame();
        void storeResults(std::string path);
        void storeRawFrames(const std::string &filePath, std::ofstream &file, int format, const char *pixFmt);
        void announceDeepY4m(const std::string &filePath) const;
        void compareViews(bool withKept);
        void check(int status) const;
        void check(int status, lfi_ctx *where) const;
        void shardOverGpus(const lfi::HostParams &params);
};
