// interpolator.cpp — see interpolator.h.  Follows the control flow of reference src/interpolator.cu:36-50, 95-137,
// 248-316: load the grid, upload it, compute offsets / weights / focus-map ids / constants on the host, optionally
// estimate the focus map, run the benchmark loop, store NN.png (+ mapK.png).
#include "interpolator.h"

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <filesystem>
#include <future>
#include <iomanip>
#include <iostream>
#include <mutex>
#include <stdexcept>
#include <thread>

#include "image_io.h"
#include "lfLoader.h"
#include "loadingbar.hpp"
#include "y4m.h"

int Interpolator::defaultDevice = 0;

Interpolator::Interpolator(std::string inputPath, int inChromaSite) : input{inputPath}, inSiteMode{inChromaSite}
{
    init();
}

Interpolator::Interpolator(std::string inputPath, int inChromaSite, MosaicInput mosaic) : input{inputPath}, inSiteMode{inChromaSite}, mosaicInput{mosaic}
{
    loadMosaic();
}

Interpolator::Interpolator(lfi::IVec2 inColsRows, lfi::IVec2 inResolution, uint32_t seed, int inDevice)
    : device{inDevice}, colsRows{inColsRows}, resolution{inResolution.x, inResolution.y, 4}
{
    check(lfi_create(device, &context));
    check(lfi_set_grid(context, colsRows.x, colsRows.y, resolution.x, resolution.y));
    check(lfi_fill_synthetic(context, seed));
    check(lfi_sync(context));
}

Interpolator::~Interpolator()
{
    if(inFramesPinned)
        lfi_free_pinned(inFrames);
    for(size_t i = 1; i < contexts.size(); i++)
        lfi_destroy(contexts[i]);
    if(context)
        lfi_destroy(context);
}

void Interpolator::check(int status) const
{
    check(status, context);
}

void Interpolator::check(int status, lfi_ctx *where) const
{
    if(status != LFI_OK)
        throw std::runtime_error(std::string("GPU error: ") + lfi_last_error(where));
}

// One context per GPU: the grid is broadcast once from the GPU it was loaded on, then every GPU gets its contiguous range of
// views (its own rows of the weight matrix; offsets are the same everywhere) — no further communication.
void Interpolator::shardOverGpus(const lfi::HostParams &params)
{
    if(contexts.empty())
    {
        contexts.push_back(context);
        for(int g = 1; g < gpuCount; g++)
        {
            lfi_ctx *extra = nullptr;
            check(lfi_create(device + g, &extra), nullptr);
            contexts.push_back(extra);
            check(lfi_set_grid(extra, colsRows.x, colsRows.y, resolution.x, resolution.y), extra);
        }
        if(gpuCount > 1)
        {
            std::cout << "Broadcasting the light field to " << gpuCount << " GPUs..." << std::endl;
            check(lfi_broadcast_grid(contexts.data(), gpuCount, 0));
        }
    }
    viewStart.assign(gpuCount + 1, 0);
    for(int g = 0; g < gpuCount; g++)
        viewStart[g + 1] = viewStart[g] + viewCount / gpuCount + (g < viewCount % gpuCount ? 1 : 0);
    const size_t n = params.offsets.size();
    for(int g = 0; g < gpuCount; g++)
    {
        lfi::HostParams part = params;
        part.views = viewStart[g + 1] - viewStart[g];
        part.weights.assign(params.weights.begin() + viewStart[g] * n, params.weights.begin() + viewStart[g + 1] * n);
        const lfi_params abi = part.abi();
        check(lfi_set_params(contexts[g], &abi), contexts[g]);
    }
}

void Interpolator::init()
{
    check(lfi_create(device, &context));
    loadGPUData();
}

bool Interpolator::isVideo() const
{
    return video != nullptr || mosaicVideo != nullptr;
}

int Interpolator::frameCount() const
{
    return video ? video->frameCount() : mosaicVideo ? mosaicVideo->frameCount() : 1;
}

int Interpolator::inputDepth() const
{
    return video ? video->videoDepth() : 8;
}

void Interpolator::setInputFrame(int t)
{
    if(t < 0 || t >= frameCount())
        throw std::runtime_error("The input has no time step " + std::to_string(t) + ": it has " + std::to_string(frameCount()) + "!");
    inputFrame = t;
}

lfi_mosaic Interpolator::mosaicMap() const
{
    lfi_mosaic m{};
    m.tiles_x = mosaicInput.tiles.x, m.tiles_y = mosaicInput.tiles.y;
    m.first_tile = 0, m.n = mosaicInput.tiles.x * mosaicInput.tiles.y;
    m.order = mosaicInput.rowsOrder ? LFI_MOSAIC_ROWS : LFI_MOSAIC_GRID;
    m.flags = mosaicInput.bottomUp ? LFI_MOSAIC_BOTTOM_UP : 0u;
    return m;
}

// The mosaic file: everything that can be refused is refused from the file alone, then the context is created.  An image goes up at once
// (one lfi_upload_mosaic), a Y4M's frames as interpolate() renders their time steps
void Interpolator::loadMosaic()
{
    const lfi::IVec2 tiles = mosaicInput.tiles;
    if(tiles.x < 1 || tiles.y < 1 || static_cast<long long>(tiles.x) * tiles.y > LFI_MAX_IMAGES)
        throw std::runtime_error("A mosaic needs CxR tiles, both at least 1 and at most " + std::to_string(LFI_MAX_IMAGES) + " in all!");
    const std::string ext = std::filesystem::path(input).extension().string();
    const bool y4m = ext == ".y4m" || ext == ".Y4M";
    lfi::Image image;
    int frameW = 0, frameH = 0;
    if(y4m)
    {
        mosaicVideo = std::make_unique<lfi::Y4mReader>(input, true);
        if(mosaicVideo->info().depth == 10)
            throw std::runtime_error("10-bit mosaics are not supported: " + input + " is C420p10, a mosaic video has to be 8-bit (C420jpeg, C420mpeg2)!");
        frameW = mosaicVideo->info().width, frameH = mosaicVideo->info().height;
    }
    else
    {
        image = lfi::loadImage(input);
        frameW = image.width, frameH = image.height;
    }
    if(frameW % tiles.x != 0 || frameH % tiles.y != 0)
        throw std::runtime_error("The mosaic " + input + " is " + std::to_string(frameW) + "x" + std::to_string(frameH) + ": that does not divide into " +
                                 std::to_string(tiles.x) + "x" + std::to_string(tiles.y) + " tiles without a remainder!");
    resolution = {frameW / tiles.x, frameH / tiles.y, 4};
    if(y4m && (resolution.x % 2 != 0 || resolution.y % 2 != 0))
        throw std::runtime_error("The tiles of the mosaic video " + input + " are " + std::to_string(resolution.x) + "x" + std::to_string(resolution.y) +
                                 ": a YUV 4:2:0 mosaic needs an even tile width and height (an odd size puts a 2x2 chroma block across two tiles)!");
    colsRows = mosaicInput.rowsOrder ? lfi::IVec2{tiles.x * tiles.y, 1} : tiles;
    check(lfi_create(device, &context));
    check(lfi_set_grid(context, colsRows.x, colsRows.y, resolution.x, resolution.y));
    if(y4m)
    {
        inSiting = lfi::y4mInputSiting(mosaicVideo->info().chroma, inSiteMode);
        if(inSiting == LFI_YUV_SITING_LEFT)
            std::cout << "The mosaic video's chroma is read as left-sited (C420mpeg2)." << std::endl;
        return;
    }
    std::cout << "Uploading the mosaic to GPU..." << std::endl;
    const lfi_mosaic m = mosaicMap();
    check(lfi_upload_mosaic(context, &m, 0, image.pixels.data(), static_cast<size_t>(frameW) * channels));
    check(lfi_upload_wait(context)); // the image's memory goes when this function returns
}

// Time step inputFrame of a Y4M mosaic: the frame read into page-locked memory as the I420 frame it is, split into the grid on the device
void Interpolator::uploadMosaicFrame()
{
    if(contexts.size() > 1)
        throw std::runtime_error("Several time steps of a light-field video work on one GPU only!");
    if(leanInputs)
        throw std::runtime_error("Lean inputs cannot be combined with a mosaic: a mosaic frame cannot be expanded straight into the planar copy of the inputs!");
    const size_t frameBytes = mosaicVideo->frameBytes();
    if(!inFrames)
    {
        inFramesPinned = lfi_alloc_pinned(frameBytes, reinterpret_cast<void **>(&inFrames)) == LFI_OK;
        if(!inFramesPinned)
        {
            inFramesPageable.resize(frameBytes);
            inFrames = inFramesPageable.data();
        }
    }
    std::cout << "Uploading time step " << inputFrame << " to GPU..." << std::endl;
    check(lfi_upload_wait(context)); // the previous step's copies have left the frame's memory
    mosaicVideo->readFrame(inputFrame, inFrames);
    const int range = inRange >= 0 ? inRange : (mosaicVideo->info().fullRange == 1 ? LFI_YUV_FULL : LFI_YUV_LIMITED);
    check(lfi_set_yuv_siting(context, inSiting, outSiting));
    lfi_yuv_surfaces surfaces{};
    check(lfi_yuv_surfaces_packed(LFI_YUV_I420, LFI_MEM_HOST, inFrames, mosaicVideo->info().width, mosaicVideo->info().height, &surfaces));
    const lfi_mosaic m = mosaicMap();
    check(lfi_upload_mosaic_yuv(context, &m, 0, inMatrix, range, inChroma, &surfaces));
    check(lfi_upload_wait(context));
    loadedFrame = inputFrame;
}

// Time step inputFrame of every camera: read into page-locked memory as the I420 frames they are, one call for the grid
void Interpolator::uploadVideoFrame()
{
    if(mosaicVideo)
        return uploadMosaicFrame();
    if(contexts.size() > 1)
        throw std::runtime_error("Several time steps of a light-field video work on one GPU only!");
    const size_t frameBytes = video->frameBytes();
    const size_t n = video->imageCount();
    if(!inFrames)
    {
        inFramesPinned = lfi_alloc_pinned(frameBytes * n, reinterpret_cast<void **>(&inFrames)) == LFI_OK;
        if(!inFramesPinned)
        {
            inFramesPageable.resize(frameBytes * n);
            inFrames = inFramesPageable.data();
        }
    }
    std::cout << "Uploading time step " << inputFrame << " to GPU..." << std::endl;
    check(lfi_upload_wait(context)); // the previous step's copies have left the frames' memory
    video->loadFrames(inputFrame, inFrames, frameBytes);
    const int range = inRange >= 0 ? inRange : (video->videoFullRange() == 1 ? LFI_YUV_FULL : LFI_YUV_LIMITED);
    check(lfi_set_yuv_siting(context, inSiting, outSiting)); // governs both calls below, lean inputs included
    if(video->videoDepth() == 10)
    {
        // C420p10: the frames are tight I010 surfaces (main.cpp refuses lean inputs with them)
        if(leanInputs)
            throw std::runtime_error("Lean inputs cannot be combined with 10-bit videos (C420p10): 10-bit frames cannot be expanded straight into the planar copy of the inputs!");
        lfi_yuv_surfaces surfaces{};
        check(lfi_yuv_surfaces_packed(LFI_YUV_I010, LFI_MEM_HOST, inFrames, resolution.x, resolution.y, &surfaces));
        surfaces.frame_stride = frameBytes;
        check(lfi_upload_images_yuv(context, 0, static_cast<int>(n), inMatrix, range, inChroma, &surfaces));
    }
    else if(inputsReleased)
    {
        // lean inputs: the context holds only the derived planar copy, the frames go straight into it
        lfi_yuv_surfaces surfaces{};
        check(lfi_yuv_surfaces_packed(LFI_YUV_I420, LFI_MEM_HOST, inFrames, resolution.x, resolution.y, &surfaces));
        surfaces.frame_stride = frameBytes;
        check(lfi_upload_images_yuv_derived(context, 0, static_cast<int>(n), inMatrix, range, inChroma, &surfaces));
    }
    else
        check(lfi_upload_images_yuv420(context, 0, static_cast<int>(n), inMatrix, range, inChroma, inFrames, frameBytes));
    check(lfi_upload_wait(context));
    loadedFrame = inputFrame;
}

void Interpolator::finish()
{
    if(y4mWriter)
    {
        std::unique_ptr<lfi::Y4mWriter> writer = std::move(y4mWriter);
        writer->close();
    }
    if(quiltY4mWriter)
    {
        std::unique_ptr<lfi::Y4mWriter> writer = std::move(quiltY4mWriter);
        writer->close();
    }
    if(rgbdY4mWriter)
    {
        std::unique_ptr<lfi::Y4mWriter> writer = std::move(rgbdY4mWriter);
        writer->close();
    }
    if(nv12File.is_open())
    {
        nv12File.close();
        if(nv12File.fail())
            throw std::runtime_error("Cannot write " + nv12Path);
    }
    if(gbrp10File.is_open())
    {
        gbrp10File.close();
        if(gbrp10File.fail())
            throw std::runtime_error("Cannot write " + gbrp10Path);
    }
    if(p010File.is_open())
    {
        p010File.close();
        if(p010File.fail())
            throw std::runtime_error("Cannot write " + p010Path);
    }
}

void Interpolator::loadGPUData()
{
    auto loader = std::make_unique<LfLoader>();
    LfLoader &lfLoader = *loader;
    lfLoader.loadData(input);
    colsRows = lfLoader.getColsRows();
    resolution = lfLoader.imageResolution();

    check(lfi_set_grid(context, colsRows.x, colsRows.y, resolution.x, resolution.y));
    if(lfLoader.isVideo())
    {
        // a light-field video: interpolate() uploads the time step it renders
        if(inSiteMode == lfi::Y4M_SITE_AUTO && !lfLoader.videoChromaAgrees())
            throw std::runtime_error("--in-chroma-site auto: the videos of " + input + " do not carry the same chroma tag (C420jpeg, C420mpeg2, ...)!");
        inSiting = lfi::y4mInputSiting(lfLoader.videoChroma(), inSiteMode);
        if(lfLoader.videoDepth() == 10)
            std::cout << "The videos hold 10-bit frames (C420p10, which carries no siting): their chroma is read as " << (inSiting == LFI_YUV_SITING_LEFT ? "left" : "centre")
                      << "-sited" << (inSiteMode == lfi::Y4M_SITE_AUTO ? " (--in-chroma-site auto: the siting of HEVC Main10 and AV1)." : ".") << std::endl;
        else if(inSiting == LFI_YUV_SITING_LEFT)
            std::cout << "The videos' chroma is read as left-sited (C420mpeg2)." << std::endl;
        else if(!lfLoader.videoCentreSited())
            std::cout << "Note: the videos are C" << lfLoader.videoChroma()
                      << "; their chroma is read as centre-sited (C420jpeg), at most a quarter pixel from where it was sampled"
                      << (inSiteMode == lfi::Y4M_SITE_AUTO ? "." : " (--in-chroma-site left or auto reads C420mpeg2 where it was sampled).") << std::endl;
        video = std::move(loader);
        return;
    }
    std::cout << "Uploading data to GPU..." << std::endl;
    LoadingBar bar(lfLoader.imageCount());
    for(int col = 0; col < colsRows.x; col++)
        for(int row = 0; row < colsRows.y; row++)
        {
            // image id = col*rows + row, the order the reference creates its surfaces in (src/interpolator.cu:106-113)
            // asynchronous: staged through page-locked slots on the library's copy stream, so the host walks on to the next image
            // while this one crosses PCIe (the reference copies synchronously: src/interpolator.cu:85-93, 106-113)
            check(lfi_upload_image_async(context, col * colsRows.y + row, lfLoader.image({col, row}).data(), static_cast<size_t>(resolution.x) * channels));
            bar.add();
        }
    check(lfi_upload_wait(context));
}

void Interpolator::interpolate(std::string outputPath, std::string trajectory, float inFocus, float inRange, std::string method, float effect, float aspect)
{
    int methodID;
    if(method == "TEN_WM")
        methodID = LFI_METHOD_TEN_WM;
    else if(method == "STD")
        methodID = LFI_METHOD_STD;
    else
        throw std::runtime_error("The specified interpolation method does not exist!");
    if(leanInputs)
    {
        // the context will hold only the planar copy of the inputs: whatever reads the RGBA planes, or needs a second context, is refused now
        if(mosaicVideo)
            throw std::runtime_error("Lean inputs cannot be combined with a mosaic: a mosaic frame cannot be expanded straight into the planar copy of the inputs!");
        if(!video)
            throw std::runtime_error("Lean inputs belong to a light-field video: the input has to be a directory of .y4m files!");
        if(inRange > 0 || autofocus || autoRange.x != 0 || autoRange.y != 0 || focusTiles.x != 0 || focusTiles.y != 0 || viewMaps)
            throw std::runtime_error("Lean inputs keep no RGBA planes: they cannot be combined with all-focus rendering (-r), autofocus, auto range, focus tiles or per-view focus maps!");
        if(viewCentred || perViewFocus)
            throw std::runtime_error("Lean inputs keep a planar copy padded for one set of shifts: they cannot be combined with view-centred shifts (-c) or a focus per view (-F)!");
        if(gpuCount > 1)
            throw std::runtime_error("Lean inputs work on one GPU only!");
    }
    if(outSiting != LFI_YUV_SITING_CENTRE && !rgbdY4mPath.empty())
        throw std::runtime_error("An RGB-D video frame cannot be left-sited: the chroma filter would mix the colour and the depth half (--chroma-site left with --rgbd-y4m)!");
    if(isVideo() && loadedFrame != inputFrame)
        uploadVideoFrame();
    if(quiltTile.x > 0 || quiltTile.y > 0)
    {
        if(!(quiltTiles.x > 0 && quiltTiles.y > 0))
            throw std::runtime_error("A quilt tile size needs a quilt (-q cols,rows)!");
        if(quiltTile.x < 1 || quiltTile.y < 1 || quiltTile.x > resolution.x || quiltTile.y > resolution.y)
            throw std::runtime_error("The quilt tile size has to be between 1x1 and the views' " + std::to_string(resolution.x) + "x" + std::to_string(resolution.y) +
                                     " pixels (views are only scaled down)!");
    }
    if(!quiltY4mPath.empty())
    {
        if(!(quiltTiles.x > 0 && quiltTiles.y > 0))
            throw std::runtime_error("A quilt video needs a quilt (-q cols,rows)!");
        if(gpuCount > 1)
            throw std::runtime_error("A quilt video frame needs every view in one context: it works on one GPU only!");
    }
    if(!rgbdY4mPath.empty())
    {
        // everything is checked before anything is rendered or written
        if(!(inRange > 0) || autofocus)
            throw std::runtime_error("An RGB-D video frame needs a focus map: all-focus rendering (-r greater than zero)!");
        if(gpuCount > 1)
            throw std::runtime_error("An RGB-D video frame reads the view and the map in one context: it works on one GPU only!");
        if(rgbdView < -1 || rgbdView >= viewCount)
            throw std::runtime_error("The view of the RGB-D video (--rgbd-view) has to be one of the " + std::to_string(viewCount) + " rendered views!");
        const lfi::IVec2 tile = rgbdTile.x > 0 ? rgbdTile : lfi::IVec2{resolution.x, resolution.y};
        if(tile.x < 1 || tile.y < 1 || tile.x > resolution.x || tile.y > resolution.y)
            throw std::runtime_error("The RGB-D tile size (--rgbd-tile) has to be between 1x1 and the views' " + std::to_string(resolution.x) + "x" +
                                     std::to_string(resolution.y) + " pixels (views are only scaled down)!");
        if(tile.x % 2 != 0 || tile.y % 2 != 0)
            throw std::runtime_error("The RGB-D tile size (--rgbd-tile) has to be even in width and height, it is " + std::to_string(tile.x) + "x" +
                                     std::to_string(tile.y) + "!");
        if(rgbdMap != 0 && rgbdMap != 1)
            throw std::runtime_error("The map of the RGB-D video (--rgbd-map) is 0 or 1!");
    }
    if(nativeSize.x != 0 || nativeSize.y != 0)
    {
        if(gpuCount > 1)
            throw std::runtime_error("A native image needs every view in one context: it works on one GPU only!");
        if(nativeSize.x < 1 || nativeSize.y < 1 || nativeSize.x > 65535 || nativeSize.y > 65535)
            throw std::runtime_error("The native image size has to be between 1x1 and 65535x65535 pixels!");
        if(nativeTile.x != 0 || nativeTile.y != 0)
            if(nativeTile.x < 1 || nativeTile.y < 1 || nativeTile.x > resolution.x || nativeTile.y > resolution.y)
                throw std::runtime_error("The native tile size has to be between 1x1 and the views' " + std::to_string(resolution.x) + "x" + std::to_string(resolution.y) +
                                         " pixels (views are only scaled down)!");
        if(nativeViews < 0 || nativeViews > viewCount)
            throw std::runtime_error("The native image cannot interlace more views than are rendered!");
        // the calibration is checked before anything is rendered
        (void)lfi::lenticularFromCalibration(nativeLens, nativeSize.x, nativeSize.y, nativeViews > 0 ? nativeViews : viewCount);
    }

    lfi::Parameterizer parameterizer(colsRows, resolution);
    // the minima of a grid of focus tiles over the search interval [inFocus, inFocus + inRange], on the first GPU
    const auto tilesOver = [&](lfi::IVec2 grid) {
        if(!(inRange > 0))
            throw std::runtime_error("Focus tiles need a search interval: a focusing range (-r) greater than zero!");
        const lfi::HostParams search = parameterizer.build(trajectory, inFocus, inRange, effect, aspect, viewCount);
        const lfi_params abi = search.abi();
        check(lfi_set_params(context, &abi));
        std::vector<lfi_focus_curve_result> found(static_cast<size_t>(std::max(grid.x, 0)) * std::max(grid.y, 0));
        if(tileSteps == LFI_FOCUS_TILE_STEPS)
            check(lfi_focus_tiles(context, grid.x, grid.y, nullptr, found.data()));
        else
            check(lfi_focus_tiles_steps(context, grid.x, grid.y, tileSteps, nullptr, found.data()));
        return found;
    };
    if(focusTiles.x != 0 || focusTiles.y != 0)
    {
        const std::vector<lfi_focus_curve_result> found = tilesOver(focusTiles);
        std::cout << "focus tiles: " << focusTiles.x << " x " << focusTiles.y << std::endl;
        for(int ty = 0; ty < focusTiles.y; ty++)
            for(int tx = 0; tx < focusTiles.x; tx++)
            {
                const lfi_focus_curve_result &r = found[static_cast<size_t>(ty) * focusTiles.x + tx];
                std::cout << "tile " << tx << " " << ty << " index " << r.best_index << " focus " << std::setprecision(9) << r.best_focus
                          << std::setprecision(6) << std::endl;
            }
    }
    if(autoRange.x != 0 || autoRange.y != 0)
    {
        if(autofocus)
            throw std::runtime_error("Auto range (an all-focus render) cannot be combined with autofocus (a fixed-focus render)!");
        const std::vector<lfi_focus_curve_result> found = tilesOver(autoRange);
        std::vector<int32_t> best(found.size());
        for(size_t t = 0; t < found.size(); t++)
            best[t] = found[t].best_index;
        const lfi::FocusAutoRange narrowed = lfi::focusAutoRange(best.data(), best.size(), inFocus, inRange, tileSteps);
        // nine significant digits: the printed values read back as floats (-f, -r) are the same floats
        std::cout << "auto-range: focus " << std::setprecision(9) << narrowed.focus << " range " << narrowed.range << std::setprecision(6)
                  << " (candidates " << narrowed.lo << ".." << narrowed.hi << ")" << std::endl;
        inFocus = narrowed.focus;
        inRange = narrowed.range;
    }
    if(autofocus)
    {
        // [inFocus, inFocus + inRange] is the search interval: the region's focus curve on the first GPU, then a fixed-focus render at its minimum
        if(perViewFocus || viewCentred || viewMaps)
            throw std::runtime_error("Autofocus cannot be combined with a focus per view (-F), view-centred shifts (-c) or per-view focus maps (--view-maps)!");
        if(!(inRange > 0))
            throw std::runtime_error("Autofocus needs a search interval: a focusing range (-r) greater than zero!");
        std::array<int, 4> r = autofocusRegion;
        if(r[0] == 0 && r[1] == 0 && r[2] == 0 && r[3] == 0)
            r = {0, 0, resolution.x, resolution.y};
        const lfi::HostParams search = parameterizer.build(trajectory, inFocus, inRange, effect, aspect, viewCount);
        const lfi_params abi = search.abi();
        check(lfi_set_params(context, &abi));
        lfi_focus_curve_result found{};
        // the whole frame over a number of candidates the tiles take, asked for explicitly: the frame as one tile (the same result by definition)
        const bool wholeFrame = autofocusRegion == std::array<int, 4>{0, 0, 0, 0};
        if(wholeFrame && autofocusStepsGiven && autofocusSteps >= 32 && autofocusSteps <= 256 && autofocusSteps % 32 == 0)
            check(lfi_focus_tiles_steps(context, 1, 1, autofocusSteps, nullptr, &found));
        else
            check(lfi_focus_curve(context, r[0], r[1], r[2], r[3], autofocusSteps, nullptr, &found));
        // nine significant digits: the printed value read back as a float (-f) is the same float
        std::cout << "autofocus: focus " << std::setprecision(9) << found.best_focus << std::setprecision(6) << " (candidate " << found.best_index << " of "
                  << autofocusSteps << ", " << found.pixels << " px)" << std::endl;
        inFocus = found.best_focus;
        inRange = 0;
    }
    focus = inFocus;
    range = inRange;
    lfi::HostParams params = parameterizer.build(trajectory, focus, range, effect, aspect, viewCount);
    if(unifiedFocusMap)
        params.flags |= LFI_FLAG_UNIFIED_FOCUS_MAP;
    if(deep)
    {
        if(inRange > 0 || perViewFocus || viewCentred || gpuCount > 1)
            throw std::runtime_error("Deep views (--deep) need a fixed-focus render with one focus and one set of shifts on one GPU!");
        params.flags |= LFI_FLAG_DEEP_VIEWS;
    }
    if(inFrame)
    {
        if(inRange > 0 || perViewFocus || viewCentred || deep || gpuCount > 1)
            throw std::runtime_error("In-frame edges (--edges in-frame) need a fixed-focus render with one focus and one set of shifts on one GPU, without --deep!");
        params.flags |= LFI_FLAG_IN_FRAME;
    }
    if(linearLight)
    {
        if(inRange > 0 || perViewFocus || viewCentred || deep || inFrame || gpuCount > 1)
            throw std::runtime_error("Linear-light blending (--light linear) needs a fixed-focus render with one focus and one set of shifts on one GPU, without --deep and --edges in-frame!");
        params.flags |= LFI_FLAG_LINEAR_LIGHT;
    }
    if(gpuCount < 1 || gpuCount > viewCount)
        throw std::runtime_error("The number of GPUs has to be between 1 and the number of views!");
    if((compareMethods || !compareDir.empty()) && gpuCount > 1)
        throw std::runtime_error("Comparing views (--compare, --compare-methods) works on one GPU only!");
    shardOverGpus(params);
    if(leanInputs && !inputsReleased)
    {
        // the first time step is on the device and its parameters are set: from here on the planar copy, built for them, is the only copy
        check(lfi_release_inputs(context));
        inputsReleased = true;
    }
    // The views never leave the library except through lfi_download_view / _quilt, which re-create the constant alpha: fixed-focus
    // TEN_WM renders therefore use the alpha-free byte-plane layout (a quarter fewer bytes written per launch, csrc/hip/blend_p3.hpp);
    // the other renders keep the reference's RGBA planes (they would pay a conversion pass).  Output files are identical.
    for(lfi_ctx *c : contexts)
        check(lfi_set_output_layout(c, (deep || inFrame || linearLight || (methodID == LFI_METHOD_TEN_WM && !(inRange > 0))) ? LFI_LAYOUT_PLANAR_RGB : LFI_LAYOUT_RGBA), c); // (deep views, in-frame edges, linear light: planar only)

    const int allFocus = inRange > 0;
    if(perViewFocus && allFocus)
        throw std::runtime_error("A focus per view cannot be combined with all-focus rendering (-r)!");
    const size_t n = params.offsets.size();
    if(mapSteps != 32 && (viewMaps || autofocus))
        throw std::runtime_error("The candidates of the focus map (--map-steps) cannot be combined with per-view focus maps (--view-maps) or autofocus: those keep their own!");
    if(viewMaps && !(viewCentred && allFocus))
        throw std::runtime_error("A focus map per view needs view-centred shifts (-c) and all-focus rendering (-r)!");
    if(viewCentred)
    {
        // every view shifted about its own camera; every GPU gets the rows of its own views
        const std::vector<float> focusVn = perViewFocus ? lfi::focusRamp(focus, focusEnd, viewCount) : std::vector<float>(viewCount, focus);
        std::vector<lfi_float2> offsetsVn;
        std::vector<lfi_int2> focusedVn;
        parameterizer.viewCentredOffsets(aspect, focusVn, parameterizer.interpretTrajectory(trajectory), offsetsVn, focusedVn);
        for(int g = 0; g < gpuCount; g++)
        {
            const int views = viewStart[g + 1] - viewStart[g];
            if(allFocus)
                check(lfi_set_view_float_offsets(contexts[g], offsetsVn.data() + viewStart[g] * n, views), contexts[g]);
            else
                check(lfi_set_view_offsets(contexts[g], focusedVn.data() + viewStart[g] * n, views), contexts[g]);
        }
    }
    else if(perViewFocus)
    {
        // every GPU gets the rows of its own views
        const std::vector<lfi_int2> rowsVn = parameterizer.viewOffsets(aspect, lfi::focusRamp(focus, focusEnd, viewCount),
                                                                        parameterizer.interpretTrajectory(trajectory));
        for(int g = 0; g < gpuCount; g++)
            check(lfi_set_view_offsets(contexts[g], rowsVn.data() + viewStart[g] * n, viewStart[g + 1] - viewStart[g]), contexts[g]);
    }
    if(allFocus && viewMaps)
    {
        // every view's map at its own camera; every GPU estimates the maps of its own views
        std::cout << "Estimating focus maps per view..." << std::endl;
        const std::vector<int32_t> ids = parameterizer.viewFocusMapIDs(parameterizer.interpretTrajectory(trajectory), viewCount);
        const int nIds = static_cast<int>(ids.size()) / viewCount;
        for(int g = 0; g < gpuCount; g++)
            check(lfi_view_focus_maps(contexts[g], ids.data() + static_cast<size_t>(viewStart[g]) * nIds, viewStart[g + 1] - viewStart[g], nIds),
                  contexts[g]);
    }
    else if(allFocus)
    {
        std::cout << "Estimating focus map..." << std::endl;
        for(lfi_ctx *c : contexts)
        {
            check(lfi_set_focus_steps(c, mapSteps), c);
            check(lfi_focus_map(c), c);
        }
    }

    if(compareMethods)
    {
        // the other method's views of the same parameters stay on the device as the references of the comparison
        std::cout << "Rendering the views to compare with (" << (methodID == LFI_METHOD_TEN_WM ? "STD" : "TEN_WM") << ")..." << std::endl;
        check(lfi_render(context, methodID == LFI_METHOD_TEN_WM ? LFI_METHOD_STD : LFI_METHOD_TEN_WM, allFocus, 0, viewCount));
        check(lfi_keep_views(context, 0, viewCount));
    }

    std::cout << "Rendering views..." << std::endl;
    std::cout << "Elapsed time: " << std::endl;
    double medianMs;
    if(gpuCount == 1)
    {
        lfi_bench_stats stats{};
        // the reference's mean includes its cold first launch; one warm-up launch is excluded here
        check(lfi_benchmark(context, methodID, allFocus, 0, viewCount, 1, static_cast<int>(kernelBenchmarkRuns), &stats));
        averageTime = stats.mean_ms;
        medianMs = stats.median_ms;
        std::cout << "Average time of " << std::to_string(kernelBenchmarkRuns) << " runs: " << stats.mean_ms << " ms" << std::endl;
        std::cout << "Median " << stats.median_ms << " ms, min " << stats.min_ms << " ms";
    }
    else
    {
        // all GPUs launch their view ranges concurrently; a run ends when the slowest GPU has finished
        const auto launchAll = [&] {
            for(int g = 0; g < gpuCount; g++)
                check(lfi_render(contexts[g], methodID, allFocus, 0, viewStart[g + 1] - viewStart[g]), contexts[g]);
            for(lfi_ctx *c : contexts)
                check(lfi_sync(c), c);
        };
        launchAll();
        std::vector<double> times;
        for(size_t i = 0; i < kernelBenchmarkRuns; i++)
        {
            const auto t0 = std::chrono::steady_clock::now();
            launchAll();
            times.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        }
        double sum = 0;
        for(double t : times)
            sum += t;
        averageTime = static_cast<float>(sum / times.size());
        std::sort(times.begin(), times.end());
        medianMs = times[times.size() / 2];
        std::cout << "Average time of " << std::to_string(kernelBenchmarkRuns) << " runs on " << gpuCount << " GPUs: " << averageTime << " ms" << std::endl;
        std::cout << "Median " << medianMs << " ms (host clock around all GPUs)";
    }
    const double seconds = medianMs / 1000.0;
    std::cout << ": " << viewCount / seconds << " views/s, "
              << static_cast<double>(viewCount) * resolution.x * resolution.y / seconds / 1e9 << " Gpix/s" << std::endl;
    if(compareMethods)
        compareViews(true);
    if(!compareDir.empty())
        compareViews(false);
    storeResults(outputPath);
}

// All views against the kept views of the other method, or against NN.png of compareDir: one lfi_compare_views call, one line per view.
void Interpolator::compareViews(bool withKept)
{
    const size_t pitch = static_cast<size_t>(resolution.x) * channels;
    const size_t imageBytes = pitch * resolution.y;
    uint8_t *references = nullptr;
    bool pinned = false;
    std::vector<uint8_t> pageable;
    if(!withKept)
    {
        std::cout << "Loading the images to compare with..." << std::endl;
        pinned = lfi_alloc_pinned(imageBytes * viewCount, reinterpret_cast<void **>(&references)) == LFI_OK;
        if(!pinned)
        {
            pageable.resize(imageBytes * viewCount);
            references = pageable.data();
        }
        try
        {
            for(int i = 0; i < viewCount; i++)
            {
                const auto fileName = std::filesystem::path(compareDir) / (std::string(((i < 10) ? "0" : "")) + std::to_string(i) + ".png");
                if(!std::filesystem::exists(fileName))
                    throw std::runtime_error("Cannot compare: " + fileName.string() + " does not exist!");
                const lfi::Image image = lfi::loadImage(fileName.string());
                if(image.width != resolution.x || image.height != resolution.y)
                    throw std::runtime_error("Cannot compare: " + fileName.string() + " is " + std::to_string(image.width) + "x" + std::to_string(image.height) +
                                             ", the views are " + std::to_string(resolution.x) + "x" + std::to_string(resolution.y) + "!");
                std::copy(image.pixels.begin(), image.pixels.end(), references + imageBytes * i);
            }
        }
        catch(...)
        {
            if(pinned)
                lfi_free_pinned(references);
            throw;
        }
    }
    std::vector<lfi_view_quality> quality(viewCount);
    lfi_quality all{};
    const int status = lfi_compare_views(context, 0, viewCount, references, pitch, imageBytes, quality.data(), &all);
    if(pinned)
        lfi_free_pinned(references);
    check(status);
    // nine significant digits, as the other printed results
    std::cout << std::setprecision(9);
    for(int i = 0; i < viewCount; i++)
        std::cout << "compare " << (i < 10 ? "0" : "") << i << " psnr " << quality[i].q.psnr_all << " ssim " << quality[i].q.ssim_all << " maxdiff "
                  << quality[i].max_abs_diff << " differing " << quality[i].differing_bytes << std::endl;
    std::cout << "compare all psnr " << all.psnr_all << " ssim " << all.ssim_all << std::setprecision(6) << std::endl;
}

void Interpolator::storeResults(std::string path)
{
    // Same files as the reference (NN.png, mapK.png: src/interpolator.cu:299-316).  The device→host copies land in a ring of
    // page-locked buffers and the PNG encoding runs on worker threads, so the GPU copy of view i+1 overlaps the compression
    // of view i (the reference downloads and encodes one view at a time on one thread).
    std::cout << "Storing results..." << std::endl;
    constexpr int MAP_COUNT{2};
    int count = viewCount;
    if(range > 0)
        count += viewMaps ? MAP_COUNT * viewCount : MAP_COUNT;
    std::filesystem::create_directories(path);
    LoadingBar bar(count);
    const size_t pitch = static_cast<size_t>(resolution.x) * channels;
    const size_t imageBytes = pitch * resolution.y;
    const int workers = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    const int slots = workers + 1;
    uint8_t *ring = nullptr;
    const bool pinned = lfi_alloc_pinned(imageBytes * slots, reinterpret_cast<void **>(&ring)) == LFI_OK;
    std::vector<uint8_t> pageable;
    if(!pinned)
    {
        pageable.resize(imageBytes * slots);
        ring = pageable.data();
    }
    std::mutex mutex;
    std::condition_variable slotFree;
    std::vector<bool> busy(slots, false);
    std::vector<std::future<void>> jobs;
    std::string firstError;
    for(int i = 0; i < count; i++)
    {
        int slot;
        {
            std::unique_lock<std::mutex> lock(mutex);
            slotFree.wait(lock, [&] { return std::find(busy.begin(), busy.end(), false) != busy.end(); });
            slot = static_cast<int>(std::find(busy.begin(), busy.end(), false) - busy.begin());
            busy[slot] = true;
        }
        uint8_t *data = ring + imageBytes * slot;
        auto fileName = std::filesystem::path(path) / (std::string(((i < 10) ? "0" : "")) + std::to_string(i) + ".png");
        if(i >= viewCount && viewMaps)
        {
            // map k of view v: map0_NN.png, map1_NN.png
            const int v = (i - viewCount) / MAP_COUNT, k = (i - viewCount) % MAP_COUNT;
            fileName = std::filesystem::path(path) / ("map" + std::to_string(k) + "_" + (v < 10 ? "0" : "") + std::to_string(v) + ".png");
            int g = 0;
            while(g + 1 < gpuCount && v >= viewStart[g + 1])
                g++;
            check(lfi_download_view_map(contexts[g], v - viewStart[g], k, data, pitch), contexts[g]);
        }
        else if(i >= viewCount)
        {
            fileName = std::filesystem::path(path) / ("map" + std::to_string(i - viewCount) + ".png");
            check(lfi_download_map(context, i - viewCount, data, pitch));
        }
        else
        {
            int g = 0;
            while(g + 1 < gpuCount && i >= viewStart[g + 1])
                g++;
            check(lfi_download_view(contexts[g], i - viewStart[g], data, pitch), contexts[g]);
        }
        jobs.push_back(std::async(std::launch::async, [&, slot, data, fileName] {
            try
            {
                lfi::writePng(fileName.string(), resolution.x, resolution.y, static_cast<int>(channels), data, pitch);
            }
            catch(const std::exception &e)
            {
                std::lock_guard<std::mutex> lock(mutex);
                if(firstError.empty())
                    firstError = e.what();
            }
            {
                std::lock_guard<std::mutex> lock(mutex);
                busy[slot] = false;
            }
            slotFree.notify_one();
        }));
        bar.add();
    }
    for(auto &job : jobs)
        job.get();
    if(pinned)
        lfi_free_pinned(ring);
    if(!firstError.empty())
        throw std::runtime_error(firstError);
    if(quiltTiles.x > 0 && quiltTiles.y > 0)
    {
        if(quiltTiles.x * quiltTiles.y > viewCount)
            throw std::runtime_error("The quilt has more tiles than rendered views!");
        std::cout << "Storing quilt..." << std::endl;
        // with a tile size every view is resized to it on the device (lfi_download_quilt_tiles_scaled): only the scaled bytes are copied
        const bool scaled = quiltTile.x > 0;
        const lfi::IVec2 tile = scaled ? quiltTile : lfi::IVec2{resolution.x, resolution.y};
        const size_t quiltPitch = static_cast<size_t>(tile.x) * channels * quiltTiles.x;
        std::vector<uint8_t> quilt(quiltPitch * tile.y * quiltTiles.y);
        // every GPU assembles the tiles of ITS views on the device and copies them into their place in the one host image
        const int tiles = quiltTiles.x * quiltTiles.y;
        for(int g = 0; g < gpuCount; g++)
        {
            const int first = viewStart[g], last = std::min(g + 1 < gpuCount ? viewStart[g + 1] : viewCount, tiles);
            if(first >= last)
                continue;
            if(scaled)
                check(lfi_download_quilt_tiles_scaled(contexts[g], quiltTiles.x, quiltTiles.y, first, last - first, 0, tile.x, tile.y, quilt.data(), quiltPitch), contexts[g]);
            else
                check(lfi_download_quilt_tiles(contexts[g], quiltTiles.x, quiltTiles.y, first, last - first, 0, quilt.data(), quiltPitch), contexts[g]);
        }
        lfi::writePng((std::filesystem::path(path) / "quilt.png").string(), tile.x * quiltTiles.x, tile.y * quiltTiles.y, static_cast<int>(channels), quilt.data(),
                      quiltPitch);
    }
    if(!quiltY4mPath.empty())
    {
        if(quiltTiles.x * quiltTiles.y > viewCount)
            throw std::runtime_error("The quilt has more tiles than rendered views!");
        std::cout << "Storing quilt video frame..." << std::endl;
        // resized and converted on the device (lfi_download_quilt_yuv): the one frame arrives as tight I420 in a page-locked buffer
        const lfi::IVec2 tile = quiltTile.x > 0 ? quiltTile : lfi::IVec2{resolution.x, resolution.y};
        const int quiltW = tile.x * quiltTiles.x, quiltH = tile.y * quiltTiles.y;
        const size_t frameBytes = lfi::y4mFrameBytes(quiltW, quiltH, yuvDepth);
        uint8_t *frame = nullptr;
        const bool framePinned = lfi_alloc_pinned(frameBytes, reinterpret_cast<void **>(&frame)) == LFI_OK;
        std::vector<uint8_t> pageableFrame;
        if(!framePinned)
        {
            pageableFrame.resize(frameBytes);
            frame = pageableFrame.data();
        }
        try
        {
            lfi_yuv_surfaces surface{};
            check(lfi_yuv_surfaces_packed(yuvDepth == 10 ? LFI_YUV_I010 : LFI_YUV_I420, LFI_MEM_HOST, frame, quiltW, quiltH, &surface));
            check(lfi_set_yuv_siting(context, inSiting, outSiting));
            check(lfi_download_quilt_yuv(context, quiltTiles.x, quiltTiles.y, 0, tile.x, tile.y, yuvMatrix, yuvRange, &surface));
            // one file for all time steps of a light-field video: opened by the first, appended to by the others, closed by finish()
            if(!quiltY4mWriter)
            {
                quiltY4mWriter = std::make_unique<lfi::Y4mWriter>(quiltY4mPath, quiltW, quiltH, y4mFps.x, y4mFps.y, yuvRange == LFI_YUV_FULL, outSiting == LFI_YUV_SITING_LEFT, yuvDepth);
                if(yuvDepth == 10)
                    announceDeepY4m(quiltY4mPath);
            }
            quiltY4mWriter->writeFrame(frame);
        }
        catch(...)
        {
            if(framePinned)
                lfi_free_pinned(frame);
            throw;
        }
        if(framePinned)
            lfi_free_pinned(frame);
    }
    if(!rgbdY4mPath.empty())
    {
        if(yuvDepth == 10)
            throw std::runtime_error("10-bit RGB-D frames are not supported: the RGB-D video is written with 8 bits per sample!");
        std::cout << "Storing RGB-D video frame..." << std::endl;
        // the view and the map resized and converted on the device (lfi_download_rgbd_yuv): the one frame arrives as tight I420 in a page-locked buffer
        const lfi::IVec2 tile = rgbdTile.x > 0 ? rgbdTile : lfi::IVec2{resolution.x, resolution.y};
        const int frameW = 2 * tile.x, frameH = tile.y;
        const size_t frameBytes = lfi::y4mFrameBytes(frameW, frameH);
        uint8_t *frame = nullptr;
        const bool framePinned = lfi_alloc_pinned(frameBytes, reinterpret_cast<void **>(&frame)) == LFI_OK;
        std::vector<uint8_t> pageableFrame;
        if(!framePinned)
        {
            pageableFrame.resize(frameBytes);
            frame = pageableFrame.data();
        }
        try
        {
            lfi_yuv_surfaces surface{};
            check(lfi_yuv_surfaces_packed(LFI_YUV_I420, LFI_MEM_HOST, frame, frameW, frameH, &surface));
            const uint32_t flags = (rgbdInvert ? LFI_RGBD_INVERT : 0u) | (viewMaps ? LFI_RGBD_VIEW_MAPS : 0u);
            check(lfi_download_rgbd_yuv(context, rgbdView >= 0 ? rgbdView : viewCount / 2, 1, rgbdMap, flags, tile.x, tile.y, yuvMatrix, yuvRange, &surface));
            // one file for all time steps of a light-field video: opened by the first, appended to by the others, closed by finish()
            if(!rgbdY4mWriter)
                rgbdY4mWriter = std::make_unique<lfi::Y4mWriter>(rgbdY4mPath, frameW, frameH, y4mFps.x, y4mFps.y, yuvRange == LFI_YUV_FULL);
            rgbdY4mWriter->writeFrame(frame);
        }
        catch(...)
        {
            if(framePinned)
                lfi_free_pinned(frame);
            throw;
        }
        if(framePinned)
            lfi_free_pinned(frame);
    }
    if(nativeSize.x > 0 && nativeSize.y > 0)
    {
        std::cout << "Storing native image..." << std::endl;
        // interlaced on the device (lfi_download_native): only the display's own pixels are copied
        const lfi::IVec2 tile = nativeTile.x > 0 ? nativeTile : lfi::IVec2{resolution.x, resolution.y};
        lfi_lenticular lens = lfi::lenticularFromCalibration(nativeLens, nativeSize.x, nativeSize.y, nativeViews > 0 ? nativeViews : viewCount);
        lens.flags |= nativeFlags;
        const size_t nativePitch = static_cast<size_t>(nativeSize.x) * channels;
        std::vector<uint8_t> native(nativePitch * nativeSize.y);
        check(lfi_download_native(context, &lens, 0, nativeSize.x, nativeSize.y, tile.x, tile.y, native.data(), nativePitch));
        lfi::writePng((std::filesystem::path(path) / "native.png").string(), nativeSize.x, nativeSize.y, static_cast<int>(channels), native.data(), nativePitch);
    }
    if(!y4mPath.empty())
    {
        std::cout << "Storing video..." << std::endl;
        // converted on the device (lfi_download_views_yuv420): every GPU's views arrive as frames in its part of one page-locked buffer
        const size_t frameBytes = lfi::y4mFrameBytes(resolution.x, resolution.y, yuvDepth);
        uint8_t *frames = nullptr;
        const bool framesPinned = lfi_alloc_pinned(frameBytes * viewCount, reinterpret_cast<void **>(&frames)) == LFI_OK;
        std::vector<uint8_t> pageableFrames;
        if(!framesPinned)
        {
            pageableFrames.resize(frameBytes * viewCount);
            frames = pageableFrames.data();
        }
        try
        {
            for(int g = 0; g < gpuCount; g++)
                check(lfi_set_yuv_siting(contexts[g], inSiting, outSiting), contexts[g]);
            for(int g = 0; g < gpuCount; g++)
            {
                if(yuvDepth == 10)
                {
                    // 10-bit: tight I010 surfaces (lfi_download_views_yuv)
                    lfi_yuv_surfaces surfaces{};
                    check(lfi_yuv_surfaces_packed(LFI_YUV_I010, LFI_MEM_HOST, frames + frameBytes * viewStart[g], resolution.x, resolution.y, &surfaces), contexts[g]);
                    if(deep)
                        surfaces.format |= LFI_YUV_DEEP; // the same surfaces, made from the deep views
                    check(lfi_download_views_yuv(contexts[g], 0, viewStart[g + 1] - viewStart[g], yuvMatrix, yuvRange, &surfaces), contexts[g]);
                    continue;
                }
                check(lfi_download_views_yuv420(contexts[g], 0, viewStart[g + 1] - viewStart[g], yuvMatrix, yuvRange, frames + frameBytes * viewStart[g], frameBytes),
                      contexts[g]);
            }
            // one file for all time steps of a light-field video: opened by the first, appended to by the others, closed by finish()
            if(!y4mWriter)
            {
                y4mWriter = std::make_unique<lfi::Y4mWriter>(y4mPath, resolution.x, resolution.y, y4mFps.x, y4mFps.y, yuvRange == LFI_YUV_FULL, outSiting == LFI_YUV_SITING_LEFT, yuvDepth);
                if(yuvDepth == 10)
                    announceDeepY4m(y4mPath);
                if(yuvDepth == 10 && deep)
                    std::cout << "deep views: the 10-bit frames of " << y4mPath << " are converted from the render's own 10-bit codes" << std::endl;
            }
            for(int i = 0; i < viewCount; i++)
                y4mWriter->writeFrame(frames + frameBytes * i);
        }
        catch(...)
        {
            if(framesPinned)
                lfi_free_pinned(frames);
            throw;
        }
        if(framesPinned)
            lfi_free_pinned(frames);
    }
    if(!nv12Path.empty())
    {
        std::cout << "Storing NV12 video..." << std::endl;
        storeRawFrames(nv12Path, nv12File, LFI_YUV_NV12, "nv12");
    }
    if(!p010Path.empty())
    {
        std::cout << "Storing P010 video..." << std::endl;
        storeRawFrames(p010Path, p010File, LFI_YUV_P010 | (deep ? LFI_YUV_DEEP : 0), "p010le");
    }
    if(!gbrp10Path.empty())
    {
        std::cout << "Storing deep views..." << std::endl;
        storeRawFrames(gbrp10Path, gbrp10File, LFI_YUV_GBRP10, "gbrp10le");
    }
}

// Y4M's C420p10 says nothing about where the chroma lies: say it here, with the option that tells ffmpeg
void Interpolator::announceDeepY4m(const std::string &filePath) const
{
    const bool left = outSiting == LFI_YUV_SITING_LEFT;
    std::cout << "10-bit video " << filePath << ": C420p10 (yuv420p10le) carries no chroma siting; the frames are " << (left ? "left" : "centre")
              << "-sited: ffmpeg -chroma_sample_location " << (left ? "left" : "center") << " -i " << filePath << std::endl;
}

// The views as raw semi-planar frames of `format` (LFI_YUV_NV12, or LFI_YUV_P010: two bytes per sample) appended to filePath: converted on
// the device into the tight layout (lfi_download_views_yuv), every GPU's views arriving in its part of one buffer
void Interpolator::storeRawFrames(const std::string &filePath, std::ofstream &file, int format, const char *pixFmt)
{
    // the semi-planar frame has the planar one's bytes; gbrp10le: three full planes of 16-bit samples
    const size_t frameBytes = format == LFI_YUV_GBRP10 ? (size_t)6 * resolution.x * resolution.y : lfi::y4mFrameBytes(resolution.x, resolution.y, format & LFI_YUV_10BIT ? 10 : 8);
    uint8_t *frames = nullptr;
    const bool framesPinned = lfi_alloc_pinned(frameBytes * viewCount, reinterpret_cast<void **>(&frames)) == LFI_OK;
    std::vector<uint8_t> pageableFrames;
    if(!framesPinned)
    {
        pageableFrames.resize(frameBytes * viewCount);
        frames = pageableFrames.data();
    }
    try
    {
        for(int g = 0; g < gpuCount; g++)
        {
            lfi_yuv_surfaces surfaces{};
            check(lfi_set_yuv_siting(contexts[g], inSiting, outSiting), contexts[g]);
            // (LFI_YUV_DEEP on P010 is a source flag: the layout is P010's)
            check(lfi_yuv_surfaces_packed(format == LFI_YUV_GBRP10 ? format : format & ~LFI_YUV_DEEP, LFI_MEM_HOST, frames + frameBytes * viewStart[g], resolution.x, resolution.y, &surfaces), contexts[g]);
            surfaces.format = format;
            check(lfi_download_views_yuv(contexts[g], 0, viewStart[g + 1] - viewStart[g], yuvMatrix, yuvRange, &surfaces), contexts[g]);
        }
        // one file for all time steps of a light-field video: opened by the first, appended to by the others, closed by finish()
        if(!file.is_open())
        {
            file.open(filePath, std::ios::binary | std::ios::trunc);
            if(!file)
                throw std::runtime_error("Cannot write " + filePath);
            if(deep && format != LFI_YUV_GBRP10)
                std::cout << "deep views: the 10-bit frames of " << filePath << " are converted from the render's own 10-bit codes" << std::endl;
            std::cout << (format == LFI_YUV_GBRP10 ? "deep views (planar 10-bit RGB)" : format & LFI_YUV_10BIT ? "P010" : "NV12") << " video " << filePath << ": ffmpeg -f rawvideo -pix_fmt " << pixFmt << " -s " << resolution.x << "x"
                      << resolution.y << " -r " << y4mFps.x;
            if(y4mFps.y != 1)
                std::cout << "/" << y4mFps.y;
            std::cout << " -i " << filePath << std::endl;
        }
        file.write(reinterpret_cast<const char *>(frames), static_cast<std::streamsize>(frameBytes * viewCount));
        if(!file)
            throw std::runtime_error("Cannot write " + filePath);
    }
    catch(...)
    {
        if(framesPinned)
            lfi_free_pinned(frames);
        throw;
    }
    if(framesPinned)
        lfi_free_pinned(frames);
}
