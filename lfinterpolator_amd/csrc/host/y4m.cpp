// y4m.cpp — see y4m.h
#include "y4m.h"

#include <stdexcept>

namespace lfi {

size_t y4mFrameBytes(int width, int height)
{
    if(width < 1 || height < 1)
        return 0;
    return static_cast<size_t>(width) * height + 2 * ((static_cast<size_t>(width) + 1) / 2) * ((static_cast<size_t>(height) + 1) / 2);
}

Y4mWriter::Y4mWriter(const std::string &path, int width, int height, int fpsNum, int fpsDen, bool fullRange) : name{path}
{
    if(width < 1 || height < 1 || fpsNum < 1 || fpsDen < 1)
        throw std::runtime_error("Y4M needs a frame size and a frame rate of at least 1 (" + path + ")");
    bytes = y4mFrameBytes(width, height);
    file = std::fopen(path.c_str(), "wb");
    if(!file)
        throw std::runtime_error("Cannot write " + path);
    if(std::fprintf(file, "YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 C420jpeg XCOLORRANGE=%s\n", width, height, fpsNum, fpsDen, fullRange ? "FULL" : "LIMITED") < 0)
    {
        std::fclose(file);
        file = nullptr;
        throw std::runtime_error("Cannot write " + path);
    }
}

Y4mWriter::~Y4mWriter()
{
    if(file)
        std::fclose(file);
}

void Y4mWriter::writeFrame(const uint8_t *frame)
{
    if(!file || !frame)
        throw std::runtime_error("Cannot write a frame to " + name);
    if(std::fwrite("FRAME\n", 1, 6, file) != 6 || std::fwrite(frame, 1, bytes, file) != bytes)
        throw std::runtime_error("Cannot write " + name);
}

void Y4mWriter::close()
{
    if(!file)
        return;
    std::FILE *f = file;
    file = nullptr;
    if(std::fclose(f) != 0)
        throw std::runtime_error("Cannot write " + name);
}

void writeY4m(const std::string &path, const uint8_t *frames, int n, size_t frameStrideBytes, int width, int height, int fpsNum, int fpsDen, bool fullRange)
{
    // checked before the file is created
    if(n < 0 || (n > 0 && (!frames || frameStrideBytes < y4mFrameBytes(width, height))))
        throw std::runtime_error("Y4M frames are missing or closer together than a frame's bytes (" + path + ")");
    Y4mWriter writer(path, width, height, fpsNum, fpsDen, fullRange);
    for(int k = 0; k < n; k++)
        writer.writeFrame(frames + frameStrideBytes * k);
    writer.close();
}

} // namespace lfi
