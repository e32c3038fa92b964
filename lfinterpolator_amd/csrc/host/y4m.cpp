// y4m.cpp — see y4m.h
#include "y4m.h"

#include <cstdlib>
#include <sstream>
#include <stdexcept>

namespace lfi {

size_t y4mFrameBytes(int width, int height, int depth)
{
    if(width < 1 || height < 1)
        return 0;
    return (static_cast<size_t>(width) * height + 2 * ((static_cast<size_t>(width) + 1) / 2) * ((static_cast<size_t>(height) + 1) / 2)) * (depth == 10 ? 2 : 1);
}

Y4mWriter::Y4mWriter(const std::string &path, int width, int height, int fpsNum, int fpsDen, bool fullRange, bool leftSited, int depth) : name{path}
{
    if(width < 1 || height < 1 || fpsNum < 1 || fpsDen < 1)
        throw std::runtime_error("Y4M needs a frame size and a frame rate of at least 1 (" + path + ")");
    if(depth != 8 && depth != 10)
        throw std::runtime_error("Y4M frames are written with 8 or 10 bits per sample (" + path + ")");
    bytes = y4mFrameBytes(width, height, depth);
    file = std::fopen(path.c_str(), "wb");
    if(!file)
        throw std::runtime_error("Cannot write " + path);
    if(std::fprintf(file, "YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 C420%s XCOLORRANGE=%s\n", width, height, fpsNum, fpsDen, depth == 10 ? "p10" : leftSited ? "mpeg2" : "jpeg", fullRange ? "FULL" : "LIMITED") < 0)
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

void writeY4m(const std::string &path, const uint8_t *frames, int n, size_t frameStrideBytes, int width, int height, int fpsNum, int fpsDen, bool fullRange,
              bool leftSited, int depth)
{
    // checked before the file is created
    if(n < 0 || (n > 0 && (!frames || frameStrideBytes < y4mFrameBytes(width, height, depth))))
        throw std::runtime_error("Y4M frames are missing or closer together than a frame's bytes (" + path + ")");
    Y4mWriter writer(path, width, height, fpsNum, fpsDen, fullRange, leftSited, depth);
    for(int k = 0; k < n; k++)
        writer.writeFrame(frames + frameStrideBytes * k);
    writer.close();
}

int y4mInputSiting(const std::string &chromaTag, int mode)
{
    if(mode == Y4M_SITE_AUTO)
        return chromaTag == "420mpeg2" || chromaTag == "420p10" ? Y4M_SITE_LEFT : Y4M_SITE_CENTRE;
    return mode == Y4M_SITE_LEFT ? Y4M_SITE_LEFT : Y4M_SITE_CENTRE;
}

namespace {

// a whole decimal number of at most 9 digits and nothing else
bool wholeNumber(const std::string &t, int &out)
{
    if(t.empty() || t.size() > 9 || t.find_first_not_of("0123456789") != std::string::npos)
        return false;
    out = std::atoi(t.c_str());
    return true;
}

} // namespace

// one line without its '\n', at most `limit` characters; eof: nothing was left to read
std::string Y4mReader::readLine(size_t limit, bool &eof)
{
    std::string line;
    eof = false;
    for(;;)
    {
        const int c = std::fgetc(file);
        if(c == EOF)
        {
            if(line.empty())
                eof = true;
            else
                throw std::runtime_error("Y4M file " + name + " ends inside a header line");
            return line;
        }
        if(c == '\n')
            return line;
        if(line.size() >= limit)
            throw std::runtime_error("Y4M file " + name + " has an overlong header line");
        line.push_back(static_cast<char>(c));
    }
}

Y4mReader::Y4mReader(const std::string &path, bool acceptDeep) : name{path}
{
    file = std::fopen(path.c_str(), "rb");
    if(!file)
        throw std::runtime_error("Cannot read " + path);
    try
    {
        bool eof = false;
        const std::string line = readLine(1024, eof);
        std::istringstream tokens(line);
        std::string token;
        if(!(tokens >> token) || token != "YUV4MPEG2")
            throw std::runtime_error(path + " is not a YUV4MPEG2 (Y4M) file");
        bool haveW = false, haveH = false;
        while(tokens >> token)
        {
            const std::string value = token.substr(1);
            switch(token[0])
            {
            case 'W':
                haveW = wholeNumber(value, header.width);
                if(!haveW)
                    throw std::runtime_error("Y4M file " + path + " has a malformed width: " + token);
                break;
            case 'H':
                haveH = wholeNumber(value, header.height);
                if(!haveH)
                    throw std::runtime_error("Y4M file " + path + " has a malformed height: " + token);
                break;
            case 'F':
            {
                const size_t cut = value.find(':');
                if(cut == std::string::npos || !wholeNumber(value.substr(0, cut), header.fpsNum) || !wholeNumber(value.substr(cut + 1), header.fpsDen))
                    throw std::runtime_error("Y4M file " + path + " has a malformed frame rate: " + token);
                break;
            }
            case 'I':
                if(value != "p" && value != "?")
                    throw std::runtime_error("Y4M file " + path + " is interlaced (" + token + "): only progressive video is read");
                break;
            case 'A':
                break; // the pixel aspect ratio changes no byte
            case 'C':
                if(acceptDeep && value == "420p10")
                {
                    header.chroma = value;
                    header.centreSited = false; // the tag carries no siting
                    header.depth = 10;
                    break;
                }
                if(value != "420jpeg" && value != "420mpeg2" && value != "420paldv" && value != "420")
                    throw std::runtime_error("Y4M file " + path + " is " + token + ": only 8-bit 4:2:0 (C420jpeg, C420mpeg2, C420paldv, C420) is read");
                header.chroma = value;
                header.centreSited = value == "420jpeg";
                header.depth = 8;
                break;
            case 'X':
                if(value == "COLORRANGE=FULL")
                    header.fullRange = 1;
                else if(value == "COLORRANGE=LIMITED")
                    header.fullRange = 0;
                break; // other extensions are ignored
            default:
                throw std::runtime_error("Y4M file " + path + " has an unknown header token: " + token);
            }
        }
        if(!haveW || !haveH || header.width < 1 || header.height < 1)
            throw std::runtime_error("Y4M file " + path + " needs a frame size of at least 1x1 (W and H)");
        bytes = y4mFrameBytes(header.width, header.height, header.depth);
        dataStart = static_cast<long long>(line.size()) + 1;
        if(std::fseek(file, 0, SEEK_END) != 0)
            throw std::runtime_error("Cannot read " + path);
        const long long size = std::ftell(file);
        // plain "FRAME\n" lines: the size decides; otherwise (parameters on the first line, or a size that is no whole number of plain
        // frames) the FRAME lines are walked
        bool plain = size == dataStart;
        if(size >= dataStart + 6)
        {
            char mark[6];
            if(std::fseek(file, static_cast<long>(dataStart), SEEK_SET) != 0 || std::fread(mark, 1, 6, file) != 6)
                throw std::runtime_error("Cannot read " + path);
            plain = std::string(mark, 6) == "FRAME\n" && (size - dataStart) % static_cast<long long>(6 + bytes) == 0;
        }
        if(plain)
            header.frames = static_cast<int>((size - dataStart) / static_cast<long long>(6 + bytes));
        else
        {
            long long at = dataStart;
            while(at < size)
            {
                if(std::fseek(file, static_cast<long>(at), SEEK_SET) != 0)
                    throw std::runtime_error("Cannot read " + path);
                const std::string frameLine = readLine(256, eof);
                if(frameLine.compare(0, 5, "FRAME") != 0 || (frameLine.size() > 5 && frameLine[5] != ' '))
                    throw std::runtime_error("Y4M file " + path + " has no FRAME line where frame " + std::to_string(offsets.size()) + " should start");
                at += static_cast<long long>(frameLine.size()) + 1;
                if(at + static_cast<long long>(bytes) > size)
                    throw std::runtime_error("Y4M file " + path + " is truncated: its last frame is incomplete");
                offsets.push_back(at);
                at += static_cast<long long>(bytes);
            }
            header.frames = static_cast<int>(offsets.size());
        }
    }
    catch(...)
    {
        std::fclose(file);
        file = nullptr;
        throw;
    }
}

Y4mReader::~Y4mReader()
{
    if(file)
        std::fclose(file);
}

void Y4mReader::readFrame(int t, uint8_t *frame)
{
    if(!frame || t < 0 || t >= header.frames)
        throw std::runtime_error("Y4M file " + name + " has no frame " + std::to_string(t) + " (it has " + std::to_string(header.frames) + ")");
    const long long at = offsets.empty() ? dataStart + static_cast<long long>(t) * static_cast<long long>(6 + bytes) + 6 : offsets[t];
    if(std::fseek(file, static_cast<long>(at), SEEK_SET) != 0 || std::fread(frame, 1, bytes, file) != bytes)
        throw std::runtime_error("Cannot read frame " + std::to_string(t) + " of " + name);
}

} // namespace lfi
