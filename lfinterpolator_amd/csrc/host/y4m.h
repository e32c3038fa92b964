// y4m.h — a YUV4MPEG2 (Y4M) writer for the I420 frames of lfi_download_views_yuv420 / lfi_render_stream_yuv420 (include/lfi.h): the
// uncompressed video file `ffmpeg -i path.y4m` and players open as it is — and a reader of such files for lfi_upload_images_yuv420.
//
//     YUV4MPEG2 W<w> H<h> F<num>:<den> Ip A1:1 C420jpeg XCOLORRANGE=LIMITED|FULL\n        the header: progressive, square pixels, 4:2:0
//     FRAME\n <frame_bytes>                                                                with centre-sited chroma (what the device computes)
//     …
// Left-sited frames (lfi_set_yuv_siting's out_siting: MPEG-2 / H.264 siting) are tagged C420mpeg2 in place of C420jpeg.
// frame_bytes = w·h + 2·((w + 1) / 2)·((h + 1) / 2): the Y plane, then Cb, then Cr, tightly packed.  The colour matrix has no header field
// in Y4M; the range goes into the XCOLORRANGE extension ffmpeg reads and writes.
// 10-bit frames (depth 10: LFI_YUV_I010, ffmpeg's yuv420p10le) are tagged C420p10: the same planes with every sample a little-endian u16
// holding the code in bits 9..0, frame_bytes doubled.  Y4M has no siting tag for them: C420p10 says nothing about where the chroma lies.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace lfi {

// w·h + 2·((w + 1) / 2)·((h + 1) / 2), twice that for depth 10; 0 for a size below 1
size_t y4mFrameBytes(int width, int height, int depth = 8);

class Y4mWriter
{
    public:
        // creates (truncates) the file and writes the header; throws std::runtime_error for a size or rate below 1 or a file that cannot be written
        // leftSited: the frames' chroma is left-sited, the header says C420mpeg2; depth 10 (else 8): I010 frames, the header says C420p10
        // whatever the siting
        Y4mWriter(const std::string &path, int width, int height, int fpsNum, int fpsDen, bool fullRange, bool leftSited = false, int depth = 8);
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
void writeY4m(const std::string &path, const uint8_t *frames, int n, size_t frameStrideBytes, int width, int height, int fpsNum, int fpsDen, bool fullRange,
              bool leftSited = false, int depth = 8);

// How the chroma of a file tagged C<chromaTag> is read under --in-chroma-site centre | left | auto: Y4M_SITE_CENTRE or Y4M_SITE_LEFT
// (= LFI_YUV_SITING_*).  auto: 420mpeg2 is left-sited, 420jpeg centre-sited; 420paldv and plain 420 have no definition here and stay centre;
// 420p10 carries no siting and is read left-sited, the siting of the codecs that make 10-bit video (HEVC Main10, AV1)
enum { Y4M_SITE_CENTRE = 0, Y4M_SITE_LEFT = 1, Y4M_SITE_AUTO = 2 };
int y4mInputSiting(const std::string &chromaTag, int mode);

// What a Y4M file's header says.  Tokens may come in any order; W and H are required, unknown X tokens are ignored.
struct Y4mInfo
{
    int width{0}, height{0};
    int fpsNum{0}, fpsDen{0}; // 0:0 — no F token
    int frames{0};
    std::string chroma{"420jpeg"}; // the C tag as written, without the C (no C token: Y4M's default, 420jpeg)
    bool centreSited{true};        // 420jpeg; 420mpeg2, 420paldv and plain 420 site their chroma up to a quarter pixel off centre
    int fullRange{-1};             // XCOLORRANGE: 1 FULL, 0 LIMITED, -1 no such token
    int depth{8};                  // 10: C420p10 (only a reader opened with acceptDeep reports it)
};

// Reads 8-bit 4:2:0 progressive Y4M files frame by frame.  Accepts C420jpeg, C420mpeg2, C420paldv and C420 (the frames have one layout;
// the tag is reported); throws std::runtime_error for any other subsampling or bit depth, interlaced material (It, Ib, Im), a size below
// 1, a malformed header or FRAME line and a truncated last frame.  Where the frames carry no parameters the number of frames comes from
// the file's size, otherwise from a walk over the FRAME lines.
class Y4mReader
{
    public:
        // acceptDeep: C420p10 files are read too (frames of twice the bytes, info().depth == 10); without it they are refused like every
        // other tag that is not 8-bit 4:2:0
        explicit Y4mReader(const std::string &path, bool acceptDeep = false);
        ~Y4mReader();
        Y4mReader(const Y4mReader &) = delete;
        Y4mReader &operator=(const Y4mReader &) = delete;

        const Y4mInfo &info() const { return header; }
        size_t frameBytes() const { return bytes; }
        int frameCount() const { return header.frames; }
        void readFrame(int t, uint8_t *frame); // frameBytes() bytes of frame t in [0, frameCount()); throws when t is outside or the read fails

    private:
        std::FILE *file{nullptr};
        std::string name;
        Y4mInfo header;
        size_t bytes{0};
        long long dataStart{0};         // offset of the first FRAME line
        std::vector<long long> offsets; // of every frame's bytes, where FRAME lines carry parameters; empty: dataStart + t·(6 + bytes) + 6
        std::string readLine(size_t limit, bool &eof);
};

} // namespace lfi
