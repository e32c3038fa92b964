// lfLoader.h — loads a cols×rows grid of same-sized images named <row>_<col>.<ext> from a directory.  A directory whose files are all
// <row>_<col>.y4m is a light-field VIDEO, one file per camera: loadData reads the headers only, loadFrames(t) one I420 frame per camera.
// Public interface source-compatible with the reference's LfLoader (reference src/lfLoader.h:7-41) with glm's vector
// types replaced by the PODs of vec.h.
#pragma once

#include <filesystem>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "vec.h"
#include "y4m.h"

class LfLoader
{
    public:
        using DataGrid = std::vector<std::vector<std::vector<uint8_t>>>;
        lfi::IVec2 getColsRows() const
        {
            return colsRows;
        }
        void loadData(std::string path);
        size_t imageSize() const
        {
            return static_cast<size_t>(resolution.x) * resolution.y * resolution.z;
        }
        lfi::IVec3 imageResolution() const
        {
            return resolution;
        }
        size_t imageCount() const
        {
            return static_cast<size_t>(colsRows.x) * colsRows.y;
        }
        const std::vector<uint8_t> &image(lfi::IVec2 colRow) const
        {
            return grid[colRow.x][colRow.y];
        }
        // a light-field video (every file a .y4m): no image() then.  The cameras agree in size and range tag; frameCount() is the shortest
        // file's.  loadFrames fills frame t of camera (col, row) at frames + (col·rows + row)·frameStrideBytes — the image ids' order
        bool isVideo() const { return !videos.empty(); }
        int frameCount() const { return frames; }
        size_t frameBytes() const { return isVideo() ? videos.front()->frameBytes() : 0; }
        int videoFullRange() const { return isVideo() ? videos.front()->info().fullRange : -1; } // XCOLORRANGE: 1, 0, -1 (no tag)
        std::string videoChroma() const { return isVideo() ? videos.front()->info().chroma : std::string(); }
        bool videoCentreSited() const { return !isVideo() || videos.front()->info().centreSited; }
        bool videoChromaAgrees() const; // every camera's file carries the same C tag
        int videoDepth() const { return isVideo() ? videos.front()->info().depth : 8; } // 10: C420p10, I010 frames (every camera's, or loadData throws)
        void loadFrames(int t, uint8_t *frames, size_t frameStrideBytes);

    private:
        lfi::IVec3 resolution{};
        lfi::IVec2 colsRows{};
        DataGrid grid;
        std::vector<std::unique_ptr<lfi::Y4mReader>> videos; // [col·rows + row]
        int frames{0};
        void openVideos(const std::string &path, const std::set<std::filesystem::path> &files);
        void initGrid(lfi::IVec2 inColsRows);
        const std::set<std::filesystem::path> listPath(std::string path) const;
        lfi::IVec2 parseFilename(std::string name) const;
        void loadImage(std::string path, lfi::IVec2 coords);
};
