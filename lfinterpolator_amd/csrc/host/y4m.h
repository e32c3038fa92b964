// y4m.h — a YUV4MPEG2 (Y4M) writer for the I420 frames of lfi_download_views_yuv420 / lfi_render_stream_yuv420 (include/lfi.h): the
// uncompressed video file `ffmpeg -i path.y4m` and players open as it is.
//
//     YUV4MPEG2 W<w> H<h> F<num>:<den> Ip A1:1 C420jpeg XCOLORRANGE=LIMITED|FULL\n        the header: progressive, square pixels, 4:2:0
//     FRAME\n <frame_bytes>                                                                with centre-sited chroma (what the device computes)
//     …
// frame_bytes = w·h + 2·((w + 1) / 2)·((h + 1) / 2): the Y plane, then Cb, then Cr, tightly packed.  The colour matrix has no header field
// in Y4M; the range goes into the XCOLORRANGE extension ffmpeg reads and writes.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>

namespace lfi {

// w·h + 2·((w + 1) / 2)·((h + 1) / 2); 0 for a size below 1
size_t y4mFrameBytes(int width, int height);

class Y4mWriter
{
    public:
        // creates (truncates) the file and writes the header; throws std::runtime_error for a size or rate below 1 or a file that cannot be written
        Y4mWriter(const std::string &path, int width, int height, int fpsNum, int fpsDen, bool fullRange);
        ~Y4mWriter();
        Y4mWriter(const Y4mWriter &) = delete;
        Y4mWriter &operator=(const Y4mWriter &) = delete;

        size_t frameBytes() const { return bytes; }
        void writeFrame(const uint8_t *frame); // "FRAME\n" and frameBytes() bytes; throws when the write fails
        void close();                          // flushes and closes; throws when that fails (the destructor closes silently)

    private:
        std::FILE *file{nullptr};
        std::string name;
        size_t bytes{0};
};

// n frames, frame k at frames + k·frameStrideBytes, as one file
void writeY4m(const std::string &path, const uint8_t *frames, int n, size_t frameStrideBytes, int width, int height, int fpsNum, int fpsDen, bool fullRange);

} // namespace lfi
