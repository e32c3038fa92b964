// lenticular.cpp — see lenticular.h.  The order of the operations below is part of the definition (tests/native_ref.py restates it).
#include "lenticular.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <stdexcept>

namespace lfi {

namespace {

// round to the nearest integer, ties away from zero, reduced mod 2³² (a negative value wraps)
uint32_t roundToPhase(double v)
{
    const double mag = v < 0.0 ? -v : v;
    if(!(mag < 4503599627370496.0)) // 2⁵²: below it mag + ½ is exact
        throw std::runtime_error("The lens calibration gives a phase step beyond 2^52 units!");
    const int64_t r = static_cast<int64_t>(mag + 0.5);
    return static_cast<uint32_t>(static_cast<uint64_t>(v < 0.0 ? -r : r));
}

} // namespace

lfi_lenticular lenticularFromCalibration(const LensCalibration &c, int out_w, int out_h, int n)
{
    if(!(c.pitch > 0.0) || !(c.dpi > 0.0) || !std::isfinite(c.pitch) || !std::isfinite(c.dpi) || !std::isfinite(c.slope) || c.slope == 0.0 ||
       !std::isfinite(c.center))
        throw std::runtime_error("A lens calibration needs pitch > 0, dpi > 0, a slope other than 0 and a finite center!");
    if(out_w < 1 || out_h < 1 || n < 1)
        throw std::runtime_error("A lens calibration needs an output of at least 1x1 pixels and at least one view!");
    const double w = out_w, h = out_h, two32 = 4294967296.0;
    const double absSlope = c.slope < 0.0 ? -c.slope : c.slope;
    const double p = ((c.pitch * w) / c.dpi) * (absSlope / std::sqrt(c.slope * c.slope + 1.0));
    const double tilt = h / (w * c.slope);
    lfi_lenticular lens{};
    lens.x_step = roundToPhase((two32 * p) / (3.0 * w));
    lens.y_step = roundToPhase(((two32 * p) * tilt) / h);
    lens.phase0 = roundToPhase(two32 * (p * (0.5 / w + (0.5 * tilt) / h) - c.center));
    lens.views = n;
    lens.flags = c.invert ? LFI_LENT_INVERT : 0u;
    return lens;
}

namespace {

// A scanner for the JSON of a calibration file: enough of the grammar to walk one object, read numbers and skip everything else.
struct JsonScanner
{
    const std::string &s;
    size_t i = 0;

    [[noreturn]] void fail(const std::string &what) const
    {
        throw std::runtime_error("The lens calibration file is not the JSON object expected: " + what + " at byte " + std::to_string(i) + "!");
    }
    void space()
    {
        while(i < s.size() && (s[i] == ' ' || s[i] == '\t' || s[i] == '\n' || s[i] == '\r'))
            i++;
    }
    bool take(char c)
    {
        space();
        if(i < s.size() && s[i] == c)
        {
            i++;
            return true;
        }
        return false;
    }
    void expect(char c, const std::string &where)
    {
        if(!take(c))
            fail(std::string("'") + c + "' expected " + where);
    }
    // a string's text; escapes are kept as written (no key taken holds one)
    std::string string(const std::string &where)
    {
        expect('"', where);
        const size_t begin = i;
        while(i < s.size() && s[i] != '"')
            i += s[i] == '\\' ? 2 : 1;
        if(i >= s.size())
            fail("unterminated string");
        return s.substr(begin, i++ - begin);
    }
    bool atNumber()
    {
        space();
        return i < s.size() && (s[i] == '-' || (s[i] >= '0' && s[i] <= '9'));
    }
    double number()
    {
        const char *begin = s.c_str() + i;
        char *end = nullptr;
        const double v = std::strtod(begin, &end);
        if(end == begin)
            fail("number expected");
        i += static_cast<size_t>(end - begin);
        return v;
    }
    // any value, its content unread
    void skip(int depth = 0)
    {
        if(depth > 64)
            fail("nesting too deep");
        space();
        if(i >= s.size())
            fail("value expected");
        if(s[i] == '"')
            (void)string("");
        else if(atNumber())
            (void)number();
        else if(s[i] == '{' || s[i] == '[')
        {
            const bool object = s[i++] == '{';
            const char close = object ? '}' : ']';
            if(take(close))
                return;
            do
            {
                if(object)
                {
                    (void)string("before a key");
                    expect(':', "after a key");
                }
                skip(depth + 1);
            } while(take(','));
            expect(close, "at the end of a nested value");
        }
        else
        {
            for(const char *word : {"true", "false", "null"})
                if(s.compare(i, std::strlen(word), word) == 0)
                {
                    i += std::strlen(word);
                    return;
                }
            fail("value expected");
        }
    }
    // the number of a taken key: x, or the "value" of {"value": x, …}; false when the entry holds neither
    bool numeric(double &out)
    {
        if(atNumber())
        {
            out = number();
            return true;
        }
        if(!take('{'))
        {
            skip();
            return false;
        }
        bool found = false;
        if(take('}'))
            return false;
        do
        {
            const std::string key = string("before a key");
            expect(':', "after a key");
            if(key == "value" && atNumber())
            {
                out = number();
                found = true;
            }
            else
                skip(1);
        } while(take(','));
        expect('}', "at the end of an entry");
        return found;
    }
};

} // namespace

LensFile lensCalibrationFromJson(const std::string &text)
{
    struct Entry
    {
        const char *key;
        bool required, found;
        double value;
    };
    Entry entries[] = {{"pitch", true, false, 0},     {"slope", true, false, 0},      {"center", true, false, 0},     {"DPI", true, false, 0},
                       {"invView", false, false, 0},  {"flipSubp", false, false, 0},  {"screenW", false, false, 0},   {"screenH", false, false, 0},
                       {"flipImageX", false, false, 0}, {"flipImageY", false, false, 0}};
    JsonScanner in{text};
    if(text.compare(0, 3, "\xEF\xBB\xBF") == 0) // a byte-order mark
        in.i = 3;
    in.expect('{', "at the start");
    if(!in.take('}'))
    {
        do
        {
            const std::string key = in.string("before a key");
            in.expect(':', "after the key \"" + key + "\"");
            Entry *entry = nullptr;
            for(Entry &e : entries)
                if(key == e.key)
                    entry = &e;
            if(!entry)
                in.skip();
            else if(!(entry->found = in.numeric(entry->value)) || !std::isfinite(entry->value))
                throw std::runtime_error("The lens calibration file gives \"" + key + "\" without a number: \"" + key + "\": x or \"" + key + "\": {\"value\": x} is expected!");
        } while(in.take(','));
        in.expect('}', "at the end");
    }
    in.space();
    if(in.i != text.size())
        in.fail("text after the object");
    for(const Entry &e : entries)
        if(e.required && !e.found)
            throw std::runtime_error(std::string("The lens calibration file has no \"") + e.key + "\": pitch, slope, center and DPI are needed!");
    for(const Entry &e : {entries[8], entries[9]})
        if(e.value != 0.0)
            throw std::runtime_error(std::string("The lens calibration file sets \"") + e.key + "\": mirrored panels are not supported!");
    for(const Entry &e : {entries[6], entries[7]})
        if(e.found && !(e.value >= 1.0 && e.value <= 1048576.0))
            throw std::runtime_error(std::string("The lens calibration file gives \"") + e.key + "\" outside 1 … 1048576 pixels!");
    LensFile file;
    file.lens.pitch = entries[0].value, file.lens.slope = entries[1].value, file.lens.center = entries[2].value, file.lens.dpi = entries[3].value;
    file.lens.invert = entries[4].value != 0.0;
    file.flags = entries[5].value != 0.0 ? LFI_LENT_BGR : 0u;
    file.screenW = static_cast<int>(entries[6].value), file.screenH = static_cast<int>(entries[7].value);
    return file;
}

LensFile lensCalibrationFromFile(const std::string &path)
{
    std::ifstream in(path, std::ios::binary);
    if(!in)
        throw std::runtime_error("The lens calibration file " + path + " cannot be opened!");
    std::stringstream text;
    text << in.rdbuf();
    if(in.bad())
        throw std::runtime_error("The lens calibration file " + path + " cannot be read!");
    return lensCalibrationFromJson(text.str());
}

} // namespace lfi
