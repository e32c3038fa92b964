// main.cpp — command line of the interpolator; flags, defaults, messages and exit codes as in reference src/main.cpp:4-57
// (-i -t -o -f -r -m -s -a -h), plus -n (views), -b (benchmark runs), -d (device), -F (focus at the last view), -c (shifts about each
// view's own camera), --autofocus (the focus found from a region's focus curve), --focus-tiles / --auto-range (the focus of every tile of a
// grid; the search interval of an all-focus render found from it), --map-steps / --tile-steps (more than 32 candidates for the focus map / the focus tiles), --compare / --compare-methods (PSNR / SSIM of all views against a
// directory of images or against the other method's render), --native / --lens / --lens-file / --lens-bgr / --native-tile / --native-views / --native-filter /
// --native-blend (the native image of a lenticular display, interlaced on the GPU, nearest or filtered), --y4m / --nv12 / --fps / --yuv-matrix / --yuv-range (the views as one YUV 4:2:0 video file, converted on
// the GPU), --yuv-depth / --p010 (10-bit frames: C420p10 Y4M files and raw P010), --quilt-y4m (the quilt as one YUV 4:2:0 video frame per time step: a quilt video), --rgbd-y4m / --rgbd-view / --rgbd-tile / --rgbd-map /
// --rgbd-invert (a view with its focus map beside it as one YUV 4:2:0 video frame per time step: RGB-D video), --chroma-site / --in-chroma-site (left-sited chroma, MPEG-2 / H.264 siting, for the frames written / read), --frames / --in-matrix / --in-range / --in-chroma (a light-field video as input: a directory of per-camera Y4M files whose frames
// become the images on the GPU), --lean-inputs (such a video at fixed focus from the planar copy of the inputs alone), --mosaic / --mosaic-order / --mosaic-bottom-up (one image or Y4M file that holds every image as a tile, split on the GPU) and --synthetic for runs without a dataset.
#include <array>
#include <iostream>
#include <memory>
#include <sstream>
#include <utility>
#include <vector>

#include "arguments.hpp"
#include "interpolator.h"

int main(int argc, char **argv)
{
    Arguments args(argc, argv);
    std::string path = static_cast<std::string>(args["-i"]);
    std::string trajectory = static_cast<std::string>(args["-t"]);
    std::string outputPath = static_cast<std::string>(args["-o"]);
    float focus = args["-f"];
    float range = args["-r"];
    std::string method = static_cast<std::string>(args["-m"]);

    std::string helpText{ "Usage:\n"
                          "Example: lfInterpolator -i /MyAmazingMachine/thoseImages -t 0.0,0.0,1.0,1.0  -o ./outputs\n"
                          "-o - output path\n"
                          "-i - folder with lf grid images - named as row_column.extension, e.g. 01_12.png\n"
                          "-t - trajectory of the camera in normalized coordinates of the grid format: startCol,startRow,endCol,endRow\n"
                          "-s - the amount of the spatial 3D effect - affects how much are views close to the virtual one prioritized (default=3.0)\n"
                          "-a - aspect ratio of the spacing of the capturing cameras in the grid (horizontal/vertical space) (default=1)\n"
                          "-m - interpolation method:\n"
                          "     STD - standard interpolation kernel (exact fp32)\n"
                          "     TEN_WM - matrix cores (fp16 MFMA)\n"
                          "The following arguments are normalized offsets of the images in shift & sum\n"
                          "-f - focusing value (default=0)\n"
                          "-r - focusing range (will be added to the focusing value) - will produce all-focused result if used\n"
                          "-F - focusing value at the last view: the focus ramps from -f at the first view to -F at the last (a focus pull; a focal stack with a single-point trajectory such as -t 0.5,0.5,0.5,0.5); not with -r\n"
                          "-c - shift the images about each view's own camera position instead of the trajectory's centre (the default, as the reference does); with -r and with -f/-F\n"
                          "--view-maps - with -c and -r: estimate every view's focus map at its own camera (the reference's focusMapCompare.sh second run, per view) instead of one map at the trajectory's centre; writes map0_NN.png / map1_NN.png per view\n"
                          "--autofocus [x0,y0,x1,y1] - find the focus of the region [x0,x1) x [y0,y1) (no value: the whole frame) and render all views at it (a fixed-focus render): -f and -r give the search interval [f, f+r] (-r required), the focus with the smallest colour dispersion over the region wins; prints \"autofocus: focus <value> ...\"; not with -F, -c, --view-maps\n"
                          "--autofocus-steps - number of focus candidates searched, 2 to 256 (default=32); given as a multiple of 32 without a region, the whole frame is searched as one focus tile (the same result, faster)\n"
                          "--focus-tiles CxR - print the focus of every tile of a grid of C columns x R rows over the frame, searched in [f, f+r] (-r required): \"focus tiles: C x R\", then \"tile <tx> <ty> index <i> focus <value>\" per tile, row by row; the render follows as usual\n"
                          "--tile-steps N - with --focus-tiles or --auto-range: the tiles choose from N candidates of [f, f+r] instead of 32, N a multiple of 32 up to 256 (indices in [0, N); about N/32 times the tiles' time); composes with --map-steps\n"
                          "--auto-range [CxR] - for all-focus renders (-r): find the interval the scene occupies from the focus tiles of a C x R grid (default 16x9) over [f, f+r] - from one candidate below the nearest tile's focus to one above the farthest's - and estimate the map and render with it in place of -f, -r; prints \"auto-range: focus <f'> range <r'> (candidates <lo>..<hi>)\"; not with --autofocus\n"
                          "--map-steps N - for all-focus renders (-r): choose every pixel's focus from N candidates of [f, f+r] instead of 32, N a multiple of 32 up to 256 (a finer focus map, about N/32 times the estimate's time); with --auto-range the tiles find the interval at 32 candidates (--tile-steps: at more) and the map is estimated with N inside it; not with --view-maps, --autofocus\n"
                          "Additional arguments:\n"
                          "-n - number of views rendered along the trajectory (default=64)\n"
                          "-b - number of timed kernel launches (default=100)\n"
                          "-d - GPU index (default=0)\n"
                          "-g - number of GPUs: the views are split over GPUs d … d+g-1, the input grid is broadcast once (default=1)\n"
                          "-q - also store quilt.png: the first cols*rows views as cols,rows tiles (e.g. 5,9 for a Looking Glass quilt)\n"
                          "--quilt-tile WxH - with -q: resize every view to a tile of W x H pixels on the GPU before quilt.png is stored (an exact area filter; downscaling only, at most the views' size), e.g. -q 5,9 --quilt-tile 819x455 for a 4096 x 4096 quilt\n"
                          "--native WxH - also store native.png: the native image of a lenticular (Looking-Glass-type) display of W x H pixels, interlaced on the GPU - every subpixel (RGB order) takes its value from the one view its position under the lens sheet selects; needs --lens; one GPU\n"
                          "--lens pitch,slope,center,dpi[,invert] - with --native: the display's calibration - lenses per inch, the slant, the phase offset in lens periods, the panel's pixels per inch, and 1 to reverse the order of the views (default 0)\n"
                          "--native-tile WxH - with --native: resize every view to a tile of W x H pixels on the GPU first (the exact area filter of --quilt-tile; at most the views' size; default: the views' size, read in place)\n"
                          "--native-views N - with --native: interlace the first N views (default: all of them)\n"
                          "--native-filter nearest|bilinear - with --native: how a tile is sampled under an output pixel's centre: nearest takes the one tile pixel there (default), bilinear weighs the four around it in 1/256 steps, as the display vendors' interlacing shaders sample a quilt; no difference where the tile has the display's size\n"
                          "--native-blend - with --native: every subpixel blends the two views nearest to its position under the lens, weighted in 1/256 steps by its distance from their centres, instead of taking the one view it falls into: no hard jumps between views; the first and the last view do not blend into each other\n"
                          "--lens-bgr - with --native: the panel's subpixels run B, G, R from left to right (native.png stays an RGB image; only which view a channel shows changes)\n"
                          "--lens-file FILE - with --native, in place of --lens: read the calibration from FILE, the JSON object such a display reports (entries \"name\": x or \"name\": {\"value\": x}): pitch, slope, center, DPI, invView (the invert of --lens), flipSubp (--lens-bgr); screenW and screenH are compared with --native and a difference is noted; a mirrored panel (flipImageX, flipImageY) is refused\n"
                          "--y4m FILE - also store the views as the frames of one YUV4MPEG2 video FILE, in view order (ffmpeg -i FILE, or any player): 8-bit YUV 4:2:0 (I420, centre-sited chroma), converted on the GPU before the download - 1.5 bytes per pixel cross PCIe instead of 4; with -g every GPU converts its own views\n"
                          "--nv12 FILE - also store the views as raw NV12 frames in FILE, in view order, tightly packed (the Y plane, then one plane of interleaved Cb/Cr): what hardware encoders take; converted on the GPU like --y4m, may be given next to it, and with --frames COUNT above 1 FILE takes all steps' views; prints the ffmpeg options that open FILE (-f rawvideo -pix_fmt nv12 -s WxH -r N)\n"
                          "--p010 FILE - also store the views as raw 10-bit P010 frames in FILE (the layout of --nv12 with every sample a little-endian 16-bit word, the code in its upper 10 bits): what Main10 hardware encoders take; converted on the GPU, may be given next to --y4m and --nv12 whatever --yuv-depth says; prints the ffmpeg options that open FILE (-f rawvideo -pix_fmt p010le -s WxH -r N)\n"
                          "--deep - with a fixed-focus render: deep views - the GPU keeps 10 bits per colour channel straight from the blend's accumulator beside the 8-bit views (the PNG files are unchanged bytes), and --p010 FILE and --y4m FILE with --yuv-depth 10 are converted from those 10-bit views instead of from the 8-bit ones: a Main10 encoder gets the render without a first quantisation. Not with -r above 0, -F, -c, --view-maps, -g above 1, 8-bit video outputs (--nv12, --y4m without --yuv-depth 10), --quilt-y4m or --rgbd-y4m\n"
                          "--edges clamp|in-frame - what a fixed-focus render does with a sample that falls outside its image: clamp (default) takes the image's edge pixel, as the reference does, which smears every image's edge across a band as wide as its shift; in-frame leaves the sample out and scales the weights of the others back to their full sum (a pixel that no image covers is black), and the PNG, --y4m, --nv12, --p010, quilt and native outputs are made of those views; fixed focus on one GPU only: not with -r above 0, -F, -c, --view-maps, --deep or -g above 1\n"
                          "--light encoded|linear - in what a fixed-focus render takes its weighted mean: encoded (default) averages the input bytes as they are (gamma-encoded values), as the reference does, which darkens out-of-focus regions and shrinks bright points; linear decodes every sample from sRGB (IEC 61966-2-1) to linear light before the sum and encodes the sum afterwards, and the PNG, --y4m, --nv12, quilt, native, RGB-D and compare outputs are made of those views; fixed focus on one GPU only: not with -r above 0, -F, -c, --view-maps, --deep, --edges in-frame or -g above 1\n"
                          "--gbrp10 FILE - with --deep: also store the deep views as raw planar 10-bit RGB frames in FILE, in view order: per frame the planes G, B, R, every sample a little-endian 16-bit word with the code in its low 10 bits; prints the ffmpeg options that open FILE (-f rawvideo -pix_fmt gbrp10le -s WxH -r N)\n"
                          "--yuv-depth 8|10 - with --y4m or --quilt-y4m: the bits per sample of the frames written (default=8). 10: the files hold I010 samples (yuv420p10le) under the tag C420p10, and an 8-bit colour survives the trip into them and back exactly; Y4M has no siting tag for 10-bit frames, so the siting in use (--chroma-site) is printed with the ffmpeg option that states it (-chroma_sample_location). Not with --rgbd-y4m: RGB-D frames are 8-bit. A light-field video whose files say C420p10 is read as 10-bit frames without any option (--in-chroma-site auto reads it left-sited and says so); not with --lean-inputs: 10-bit frames cannot go straight into the planar copy\n"
                          "--quilt-y4m FILE - with -q: also store the quilt (scaled by --quilt-tile) as one frame of the YUV4MPEG2 video FILE, resized and converted to 8-bit YUV 4:2:0 on the GPU in one pass (even tile sizes) - with --frames FIRST:COUNT one frame per time step: a quilt video, what holographic players take; one GPU only\n"
                          "--rgbd-y4m FILE - with -r: also store one view with its focus map beside it as one frame of the YUV4MPEG2 video FILE, twice the tile's width: the colour left, the depth right (RGB-D, what holographic players and 2D-plus-depth displays take), both resized and converted to 8-bit YUV 4:2:0 on the GPU in one pass; the depth is the map's value as grey, and displays take white as near; with -c --view-maps the view's own map is used; with --frames FIRST:COUNT one frame per time step: an RGB-D video; one GPU only\n"
                          "--rgbd-view N - with --rgbd-y4m: the view stored (default: the middle one, views/2)\n"
                          "--rgbd-tile WxH - with --rgbd-y4m: resize the view and the map to W x H pixels each (the exact area filter of --quilt-tile; both even, at most the views' size; default: the views' size)\n"
                          "--rgbd-map 0|1 - with --rgbd-y4m: the map stored, 0 as estimated or 1 filtered (default=1)\n"
                          "--rgbd-invert - with --rgbd-y4m: store 255 minus the map's value, which swaps the near and the far end (inverted before the resize)\n"
                          "--fps N[:D] - with --y4m, --nv12, --quilt-y4m or --rgbd-y4m: the frame rate N/D frames per second (default=30:1)\n"
                          "--yuv-matrix 709|601 - with --y4m, --nv12, --quilt-y4m or --rgbd-y4m: the colour matrix, BT.709 or BT.601 (default=709)\n"
                          "--yuv-range limited|full - with --y4m, --nv12, --quilt-y4m or --rgbd-y4m: limited (Y 16..235, chroma 16..240) or full (0..255) range (default=limited)\n"
                          "--frames FIRST[:COUNT] - with -i a directory of <row>_<col>.y4m files (a light-field video, one 8-bit YUV 4:2:0 file per camera): render time steps FIRST ... FIRST+COUNT-1 (default=0:1); the frames cross PCIe as they are, 1.5 bytes per pixel, and become the images on the GPU; with COUNT above 1 every step's files go to <-o>/fTTTT/ and --y4m FILE takes all steps' views in step order (with -n 1: the video of the moving scene from one virtual camera); not with --compare, --compare-methods or -g above 1 then\n"
                          "--in-matrix 709|601 - with a light-field video: the colour matrix of its files (default=709)\n"
                          "--in-range limited|full - with a light-field video: the range of its files (default: their XCOLORRANGE tag, else limited)\n"
                          "--in-chroma bilinear|nearest - with a light-field video: how chroma is brought to full resolution (default=bilinear, the triangle filter of centre-sited chroma)\n"
                          "--in-chroma-site centre|left|auto - with a light-field video: where its chroma samples lie. centre (default): between the two columns and the two rows of their 2x2 block, as JPEG and MPEG-1 site them (C420jpeg). left: on the even column, between the two rows, as MPEG-2, H.264, HEVC and AV1 site them (C420mpeg2). auto: by the files' C tag - C420mpeg2 left, C420jpeg centre, C420paldv and plain C420 centre with a note; every camera's file must carry the same tag then\n"
                          "--chroma-site centre|left - with --y4m, --nv12 or --quilt-y4m: the chroma siting of the frames written (default=centre, C420jpeg). left is what hardware encoders assume of untagged NV12 and what H.264 and its successors signal by default; the Y4M files then say C420mpeg2, and a quilt video takes two passes on the GPU for even tile sizes too. Not with --rgbd-y4m\n"
                          "--lean-inputs - with a light-field video rendered at fixed focus: after the first time step the GPU keeps only the planar copy of the inputs (3 bytes per pixel and image instead of 7) and every later step's frames are expanded straight into it in one pass; the files written are the same; not with -r, -F, -c, --autofocus, --auto-range, --focus-tiles, --view-maps, -g above 1 or --synthetic\n"
                          "--compare DIR - after the render, compare every view with DIR/NN.png (the names -o writes; same size) on the GPU, all views in one pass: prints \"compare NN psnr <dB> ssim <index> maxdiff <largest byte difference> differing <colour bytes that differ>\" per view, then \"compare all psnr ... ssim ...\"; one GPU\n"
                          "--compare-methods - render the views with the other method first (STD if -m TEN_WM, TEN_WM if -m STD; same parameters), keep them on the GPU, render with -m and compare the two there; prints the lines of --compare; the stored images are those of -m; one GPU; not with --compare\n"
                          "--mosaic CxR - -i is ONE file that holds every image as a tile of a frame of C x R tiles, split into the grid on the GPU: an image (PNG, JPEG, PPM; e.g. a quilt) or a .y4m whose every frame is such a frame - a light-field video in one stream: frame t is time step t under --frames, --in-matrix, --in-range, --in-chroma and --in-chroma-site apply (auto reads the file's tag), the output is that of a directory of per-camera videos. The image size is the frame's divided by the tiles (a remainder is an error; for a .y4m an odd quotient too). 10-bit .y4m mosaics (C420p10) are not supported; not with --lean-inputs (a mosaic frame cannot go straight into the planar copy) or --synthetic\n"
                          "--mosaic-order grid|rows - with --mosaic: grid (default): the tile in column c and row r is the camera of the file <r>_<c> of a C x R grid. rows: the tiles in reading order are the images of a (C*R) x 1 grid - the order of -q's quilt\n"
                          "--mosaic-bottom-up - with --mosaic: the tile rows count from the frame's bottom, as Looking-Glass quilts do\n"
                          "--synthetic cols,rows,width,height[,seed] - use a generated light field instead of -i\n"
                          "--unified-map - all-focus TEN_WM reads the filtered focus map like STD (the reference reads the unfiltered one)\n"
                        };
    if(args.printHelpIfPresent(helpText))
        return 0;

    float effect = static_cast<float>(args["-s"]);
    if(effect <= 0)
        effect = 3;

    float aspect = static_cast<float>(args["-a"]);
    if(aspect <= 0)
        aspect = 1;

    const bool synthetic = static_cast<bool>(args["--synthetic"]);
    if((!args["-i"] && !synthetic) || !args["-t"] || !args["-o"] || !args["-m"])
    {
        std::cerr << "Missing required parameters. Use -h for help." << std::endl;
        return EXIT_FAILURE;
    }

    if(args["--lean-inputs"])
    {
        // the context keeps only the planar copy of the inputs: nothing that reads the RGBA planes, pads the copy for other shifts or needs a
        // second context
        const std::pair<bool, const char *> refused[] = {
            {synthetic, "--synthetic (it needs a light-field video: -i with a directory of .y4m files)"},
            {static_cast<bool>(args["--mosaic"]), "--mosaic (a mosaic frame cannot be expanded straight into the planar copy of the inputs: use a directory of per-camera .y4m files)"},
            {static_cast<bool>(args["--autofocus"]), "--autofocus (the focus curve reads the RGBA planes)"},
            {static_cast<bool>(args["--auto-range"]), "--auto-range (the focus tiles read the RGBA planes)"},
            {static_cast<bool>(args["--focus-tiles"]), "--focus-tiles (the focus tiles read the RGBA planes)"},
            {static_cast<bool>(args["--view-maps"]), "--view-maps (per-view focus maps read the RGBA planes)"},
            {args["-r"] && range > 0, "-r above 0 (all-focus rendering reads the RGBA planes)"},
            {static_cast<bool>(args["-c"]), "-c (the planar copy is padded for one set of shifts)"},
            {static_cast<bool>(args["-F"]), "-F (the planar copy is padded for one set of shifts)"},
            {args["-g"] && static_cast<int>(args["-g"]) > 1, "-g above 1 (it works in one context)"},
        };
        for(const auto &[given, what] : refused)
            if(given)
            {
                std::cerr << "--lean-inputs (only the planar copy of the inputs stays on the GPU) cannot be combined with " << what << "." << std::endl;
                return EXIT_FAILURE;
            }
    }

    if((args["--mosaic-order"] || args["--mosaic-bottom-up"]) && !args["--mosaic"])
    {
        std::cerr << "--mosaic-order and --mosaic-bottom-up belong to a mosaic: they need --mosaic CxR." << std::endl;
        return EXIT_FAILURE;
    }
    if(args["--mosaic"] && synthetic)
    {
        std::cerr << "--mosaic splits the file given with -i: it cannot be combined with --synthetic." << std::endl;
        return EXIT_FAILURE;
    }
    bool mosaicRows = false;
    if(args["--mosaic-order"])
    {
        const std::string text = static_cast<std::string>(args["--mosaic-order"]);
        if(text != "grid" && text != "rows")
        {
            std::cerr << "--mosaic-order expects grid or rows." << std::endl;
            return EXIT_FAILURE;
        }
        mosaicRows = text == "rows";
    }

    if(args["--autofocus"] && (args["-F"] || args["-c"] || args["--view-maps"]))
    {
        std::cerr << "--autofocus (one focus found for all views) cannot be combined with -F, -c or --view-maps." << std::endl;
        return EXIT_FAILURE;
    }

    if(args["--autofocus"] && !(args["-r"] && range > 0))
    {
        std::cerr << "--autofocus searches the interval [f, f+r]: it needs -r with a value greater than zero." << std::endl;
        return EXIT_FAILURE;
    }

    if(args["--autofocus-steps"] && !args["--autofocus"])
    {
        std::cerr << "--autofocus-steps needs --autofocus." << std::endl;
        return EXIT_FAILURE;
    }

    if((args["--focus-tiles"] || args["--auto-range"]) && !(args["-r"] && range > 0))
    {
        std::cerr << "--focus-tiles and --auto-range search the interval [f, f+r]: they need -r with a value greater than zero." << std::endl;
        return EXIT_FAILURE;
    }

    if(args["--tile-steps"])
    {
        const int steps = static_cast<int>(args["--tile-steps"]);
        if(!args["--focus-tiles"] && !args["--auto-range"])
        {
            std::cerr << "--tile-steps (the candidates of the focus tiles) needs --focus-tiles or --auto-range." << std::endl;
            return EXIT_FAILURE;
        }
        if(steps < 32 || steps > 256 || steps % 32 != 0)
        {
            std::cerr << "--tile-steps expects a multiple of 32 from 32 to 256." << std::endl;
            return EXIT_FAILURE;
        }
    }

    if(args["--auto-range"] && args["--autofocus"])
    {
        std::cerr << "--auto-range (an all-focus render) cannot be combined with --autofocus (a fixed-focus render)." << std::endl;
        return EXIT_FAILURE;
    }

    if(args["--map-steps"])
    {
        const int steps = static_cast<int>(args["--map-steps"]);
        if(!args["-r"])
        {
            std::cerr << "--map-steps (the candidates of the focus map) needs -r (all-focus rendering)." << std::endl;
            return EXIT_FAILURE;
        }
        if(args["--view-maps"] || args["--autofocus"])
        {
            std::cerr << "--map-steps cannot be combined with --view-maps (per-view maps keep 32 candidates) or --autofocus (--autofocus-steps sets its candidates)." << std::endl;
            return EXIT_FAILURE;
        }
        if(steps < 32 || steps > 256 || steps % 32 != 0)
        {
            std::cerr << "--map-steps expects a multiple of 32 from 32 to 256." << std::endl;
            return EXIT_FAILURE;
        }
    }

    if(args["--quilt-tile"] && !args["-q"])
    {
        std::cerr << "--quilt-tile sets the tile size of the quilt: it needs -q cols,rows." << std::endl;
        return EXIT_FAILURE;
    }

    if(args["--lens"] && args["--lens-file"])
    {
        std::cerr << "--lens and --lens-file both give the display's calibration: use one of them." << std::endl;
        return EXIT_FAILURE;
    }

    if(static_cast<bool>(args["--native"]) != (args["--lens"] || args["--lens-file"]))
    {
        std::cerr << "--native (the display's size) and --lens or --lens-file (its calibration) describe one display: give both." << std::endl;
        return EXIT_FAILURE;
    }

    if((args["--native-tile"] || args["--native-views"]) && !args["--native"])
    {
        std::cerr << "--native-tile and --native-views belong to the native image: they need --native WxH." << std::endl;
        return EXIT_FAILURE;
    }

    if((args["--native-filter"] || args["--native-blend"] || args["--lens-bgr"]) && !args["--native"])
    {
        std::cerr << "--native-filter, --native-blend and --lens-bgr belong to the native image: they need --native WxH." << std::endl;
        return EXIT_FAILURE;
    }

    uint32_t nativeFlags = 0;
    if(args["--native-filter"])
    {
        const std::string text = static_cast<std::string>(args["--native-filter"]);
        if(text != "nearest" && text != "bilinear")
        {
            std::cerr << "--native-filter expects nearest or bilinear." << std::endl;
            return EXIT_FAILURE;
        }
        nativeFlags |= text == "bilinear" ? LFI_LENT_BILINEAR : 0u;
    }
    if(args["--native-blend"])
        nativeFlags |= LFI_LENT_BLEND;
    if(args["--lens-bgr"])
        nativeFlags |= LFI_LENT_BGR;

    lfi::LensFile lensFile;
    if(args["--lens-file"])
    {
        try
        {
            if(static_cast<std::string>(args["--lens-file"]).empty())
                throw std::runtime_error("--lens-file needs the name of the calibration file to read.");
            lensFile = lfi::lensCalibrationFromFile(static_cast<std::string>(args["--lens-file"]));
        }
        catch(const std::exception &e)
        {
            std::cerr << "--lens-file: " << e.what() << std::endl;
            return EXIT_FAILURE;
        }
        nativeFlags |= lensFile.flags;
    }

    if(args["--native"] && args["-g"] && static_cast<int>(args["-g"]) > 1)
    {
        std::cerr << "--native needs every view in one context: it works on one GPU only (-g 1)." << std::endl;
        return EXIT_FAILURE;
    }

    if(args["--quilt-y4m"] && !args["-q"])
    {
        std::cerr << "--quilt-y4m stores the quilt as a video frame: it needs -q cols,rows." << std::endl;
        return EXIT_FAILURE;
    }

    if(args["--quilt-y4m"] && static_cast<std::string>(args["--quilt-y4m"]).empty())
    {
        std::cerr << "--quilt-y4m needs the name of the video file to write." << std::endl;
        return EXIT_FAILURE;
    }

    if(args["--quilt-y4m"] && args["-g"] && static_cast<int>(args["-g"]) > 1)
    {
        std::cerr << "--quilt-y4m needs every view in one context, which assembles the frame: it works on one GPU only (-g 1)." << std::endl;
        return EXIT_FAILURE;
    }

    if((args["--rgbd-view"] || args["--rgbd-tile"] || args["--rgbd-map"] || args["--rgbd-invert"]) && !args["--rgbd-y4m"])
    {
        std::cerr << "--rgbd-view, --rgbd-tile, --rgbd-map and --rgbd-invert belong to the RGB-D video: they need --rgbd-y4m FILE." << std::endl;
        return EXIT_FAILURE;
    }

    int rgbdView = -1, rgbdMap = 1, rgbdTileW = 0, rgbdTileH = 0;
    if(args["--rgbd-y4m"])
    {
        if(!(args["-r"] && range > 0) || args["--autofocus"])
        {
            std::cerr << "--rgbd-y4m stores a view beside its focus map: it needs -r with a value greater than zero (an all-focus render, which estimates the map)." << std::endl;
            return EXIT_FAILURE;
        }
        if(static_cast<std::string>(args["--rgbd-y4m"]).empty())
        {
            std::cerr << "--rgbd-y4m needs the name of the video file to write." << std::endl;
            return EXIT_FAILURE;
        }
        if(args["-g"] && static_cast<int>(args["-g"]) > 1)
        {
            std::cerr << "--rgbd-y4m reads the view and the map in one context: it works on one GPU only (-g 1)." << std::endl;
            return EXIT_FAILURE;
        }
        // whole numbers and nothing else
        const auto whole = [](const std::string &t, int &out) {
            if(t.empty() || t.size() > 9 || t.find_first_not_of("0123456789") != std::string::npos)
                return false;
            out = std::stoi(t);
            return true;
        };
        if(args["--rgbd-tile"])
        {
            const std::string text = static_cast<std::string>(args["--rgbd-tile"]);
            const size_t cut = text.find_first_of("xX");
            if(cut == std::string::npos || !whole(text.substr(0, cut), rgbdTileW) || !whole(text.substr(cut + 1), rgbdTileH) || rgbdTileW < 1 || rgbdTileH < 1)
            {
                std::cerr << "--rgbd-tile expects WxH, the tile's width x height in pixels, both at least 1." << std::endl;
                return EXIT_FAILURE;
            }
            if(rgbdTileW % 2 != 0 || rgbdTileH % 2 != 0)
            {
                std::cerr << "--rgbd-tile expects an even width and an even height: no 2x2 chroma block of the frame may straddle the colour and the depth half." << std::endl;
                return EXIT_FAILURE;
            }
        }
        const int views = args["-n"] ? static_cast<int>(args["-n"]) : LFI_REFERENCE_VIEWS;
        if(args["--rgbd-view"] && (!whole(static_cast<std::string>(args["--rgbd-view"]), rgbdView) || rgbdView >= views))
        {
            std::cerr << "--rgbd-view expects the index of a rendered view, 0 to " << views - 1 << " (-n views)." << std::endl;
            return EXIT_FAILURE;
        }
        if(args["--rgbd-map"])
        {
            const std::string text = static_cast<std::string>(args["--rgbd-map"]);
            if(text != "0" && text != "1")
            {
                std::cerr << "--rgbd-map expects 0 (the map as estimated) or 1 (filtered)." << std::endl;
                return EXIT_FAILURE;
            }
            rgbdMap = text == "1";
        }
    }

    if((args["--fps"] || args["--yuv-matrix"] || args["--yuv-range"]) && !args["--y4m"] && !args["--nv12"] && !args["--p010"] && !args["--quilt-y4m"] && !args["--rgbd-y4m"])
    {
        std::cerr << "--fps, --yuv-matrix and --yuv-range belong to the video file: they need --y4m FILE, --nv12 FILE, --p010 FILE, --quilt-y4m FILE or --rgbd-y4m FILE." << std::endl;
        return EXIT_FAILURE;
    }

    int yuvDepth = 8;
    if(args["--yuv-depth"])
    {
        const std::string text = static_cast<std::string>(args["--yuv-depth"]);
        if(text != "8" && text != "10")
        {
            std::cerr << "--yuv-depth expects 8 or 10." << std::endl;
            return EXIT_FAILURE;
        }
        yuvDepth = text == "10" ? 10 : 8;
        if(!args["--y4m"] && !args["--quilt-y4m"] && !args["--rgbd-y4m"])
        {
            std::cerr << "--yuv-depth belongs to the Y4M file: it needs --y4m FILE or --quilt-y4m FILE (--p010 FILE is 10-bit by itself)." << std::endl;
            return EXIT_FAILURE;
        }
        if(yuvDepth == 10 && args["--rgbd-y4m"])
        {
            std::cerr << "--yuv-depth 10 cannot be combined with --rgbd-y4m: 10-bit RGB-D frames are not supported, the depth half is made for 8-bit luma." << std::endl;
            return EXIT_FAILURE;
        }
    }

    if(args["--p010"] && static_cast<std::string>(args["--p010"]).empty())
    {
        std::cerr << "--p010 needs the name of the video file to write." << std::endl;
        return EXIT_FAILURE;
    }

    if(args["--gbrp10"] && !args["--deep"])
    {
        std::cerr << "--gbrp10 stores the deep views: it needs --deep." << std::endl;
        return EXIT_FAILURE;
    }
    if(args["--gbrp10"] && static_cast<std::string>(args["--gbrp10"]).empty())
    {
        std::cerr << "--gbrp10 needs the name of the file to write." << std::endl;
        return EXIT_FAILURE;
    }
    if(args["--deep"])
    {
        // deep views: one fixed-focus kernel in one context, whose 10-bit planes only the 10-bit outputs read
        const std::pair<bool, const char *> refused[] = {
            {args["-r"] && range > 0, "-r above 0 (deep views need a fixed-focus render)"},
            {static_cast<bool>(args["-F"]), "-F (a focus per view is not rendered deep)"},
            {static_cast<bool>(args["-c"]), "-c (view-centred shifts are not rendered deep)"},
            {static_cast<bool>(args["--view-maps"]), "--view-maps (all-focus rendering is not rendered deep)"},
            {args["-g"] && static_cast<int>(args["-g"]) > 1, "-g above 1 (it works in one context)"},
            {static_cast<bool>(args["--nv12"]), "--nv12 (an 8-bit video: use --p010)"},
            {args["--y4m"] && yuvDepth != 10, "--y4m at 8 bits (an 8-bit video: add --yuv-depth 10)"},
            {static_cast<bool>(args["--quilt-y4m"]), "--quilt-y4m (deep quilts are not supported)"},
            {static_cast<bool>(args["--rgbd-y4m"]), "--rgbd-y4m (RGB-D frames are 8-bit)"},
        };
        for(const auto &[given, what] : refused)
            if(given)
            {
                std::cerr << "--deep (10-bit views straight from the blend's accumulator) cannot be combined with " << what << "." << std::endl;
                return EXIT_FAILURE;
            }
    }

    bool inFrameEdges = false;
    if(args["--edges"])
    {
        const std::string text = static_cast<std::string>(args["--edges"]);
        if(text != "clamp" && text != "in-frame")
        {
            std::cerr << "--edges expects clamp or in-frame." << std::endl;
            return EXIT_FAILURE;
        }
        inFrameEdges = text == "in-frame";
    }
    if(inFrameEdges)
    {
        // in-frame edges: one fixed-focus kernel in one context
        const std::pair<bool, const char *> refused[] = {
            {args["-r"] && range > 0, "-r above 0 (in-frame edges need a fixed-focus render)"},
            {static_cast<bool>(args["-F"]), "-F (a focus per view is not rendered in frame)"},
            {static_cast<bool>(args["-c"]), "-c (view-centred shifts are not rendered in frame)"},
            {static_cast<bool>(args["--view-maps"]), "--view-maps (all-focus rendering is not rendered in frame)"},
            {static_cast<bool>(args["--deep"]), "--deep (deep in-frame views are not supported)"},
            {args["-g"] && static_cast<int>(args["-g"]) > 1, "-g above 1 (it works in one context)"},
        };
        for(const auto &[given, what] : refused)
            if(given)
            {
                std::cerr << "--edges in-frame (out-of-frame samples left out, weights renormalised) cannot be combined with " << what << "." << std::endl;
                return EXIT_FAILURE;
            }
    }

    bool linearLight = false;
    if(args["--light"])
    {
        const std::string text = static_cast<std::string>(args["--light"]);
        if(text != "encoded" && text != "linear")
        {
            std::cerr << "--light expects encoded or linear." << std::endl;
            return EXIT_FAILURE;
        }
        linearLight = text == "linear";
    }
    if(linearLight)
    {
        // linear-light blending: one fixed-focus kernel in one context
        const std::pair<bool, const char *> refused[] = {
            {args["-r"] && range > 0, "-r above 0 (linear-light blending needs a fixed-focus render)"},
            {static_cast<bool>(args["-F"]), "-F (a focus per view is not blended in linear light)"},
            {static_cast<bool>(args["-c"]), "-c (view-centred shifts are not blended in linear light)"},
            {static_cast<bool>(args["--view-maps"]), "--view-maps (all-focus rendering is not blended in linear light)"},
            {static_cast<bool>(args["--deep"]), "--deep (deep linear-light views are not supported)"},
            {inFrameEdges, "--edges in-frame (in-frame linear-light blending is not supported)"},
            {args["-g"] && static_cast<int>(args["-g"]) > 1, "-g above 1 (it works in one context)"},
        };
        for(const auto &[given, what] : refused)
            if(given)
            {
                std::cerr << "--light linear (samples decoded from sRGB before the sum, the sum encoded) cannot be combined with " << what << "." << std::endl;
                return EXIT_FAILURE;
            }
    }

    int outSiting = LFI_YUV_SITING_CENTRE;
    if(args["--chroma-site"])
    {
        const std::string text = static_cast<std::string>(args["--chroma-site"]);
        if(text != "centre" && text != "left")
        {
            std::cerr << "--chroma-site expects centre or left." << std::endl;
            return EXIT_FAILURE;
        }
        if(!args["--y4m"] && !args["--nv12"] && !args["--p010"] && !args["--quilt-y4m"] && !args["--rgbd-y4m"])
        {
            std::cerr << "--chroma-site belongs to the video file: it needs --y4m FILE, --nv12 FILE, --p010 FILE or --quilt-y4m FILE." << std::endl;
            return EXIT_FAILURE;
        }
        outSiting = text == "left" ? LFI_YUV_SITING_LEFT : LFI_YUV_SITING_CENTRE;
        if(outSiting == LFI_YUV_SITING_LEFT && args["--rgbd-y4m"])
        {
            std::cerr << "--chroma-site left cannot be combined with --rgbd-y4m: the left-sited chroma filter would mix the colour and the depth half of the frame." << std::endl;
            return EXIT_FAILURE;
        }
    }

    if(args["--y4m"] && static_cast<std::string>(args["--y4m"]).empty())
    {
        std::cerr << "--y4m needs the name of the video file to write." << std::endl;
        return EXIT_FAILURE;
    }

    if(args["--nv12"] && static_cast<std::string>(args["--nv12"]).empty())
    {
        std::cerr << "--nv12 needs the name of the video file to write." << std::endl;
        return EXIT_FAILURE;
    }

    int fpsNum = 30, fpsDen = 1;
    if(args["--fps"])
    {
        // N or N:D, both whole numbers of at least 1 and nothing else
        const std::string text = static_cast<std::string>(args["--fps"]);
        const size_t cut = text.find(':');
        const auto whole = [](const std::string &t, int &out) {
            if(t.empty() || t.size() > 9 || t.find_first_not_of("0123456789") != std::string::npos)
                return false;
            out = std::stoi(t);
            return out >= 1;
        };
        fpsDen = 1;
        if(!whole(text.substr(0, cut), fpsNum) || (cut != std::string::npos && !whole(text.substr(cut + 1), fpsDen)))
        {
            std::cerr << "--fps expects N or N:D, whole numbers of at least 1 (e.g. 30 or 30000:1001)." << std::endl;
            return EXIT_FAILURE;
        }
    }

    int yuvMatrix = LFI_YUV_BT709, yuvRange = LFI_YUV_LIMITED;
    if(args["--yuv-matrix"])
    {
        const std::string text = static_cast<std::string>(args["--yuv-matrix"]);
        if(text != "709" && text != "601")
        {
            std::cerr << "--yuv-matrix expects 709 or 601." << std::endl;
            return EXIT_FAILURE;
        }
        yuvMatrix = text == "601" ? LFI_YUV_BT601 : LFI_YUV_BT709;
    }
    if(args["--yuv-range"])
    {
        const std::string text = static_cast<std::string>(args["--yuv-range"]);
        if(text != "limited" && text != "full")
        {
            std::cerr << "--yuv-range expects limited or full." << std::endl;
            return EXIT_FAILURE;
        }
        yuvRange = text == "full" ? LFI_YUV_FULL : LFI_YUV_LIMITED;
    }

    int firstFrame = 0, frameSteps = 1;
    if(args["--frames"])
    {
        // FIRST or FIRST:COUNT, whole numbers, COUNT at least 1
        const std::string text = static_cast<std::string>(args["--frames"]);
        const size_t cut = text.find(':');
        const auto whole = [](const std::string &t, int &out) {
            if(t.empty() || t.size() > 9 || t.find_first_not_of("0123456789") != std::string::npos)
                return false;
            out = std::stoi(t);
            return true;
        };
        if(!whole(text.substr(0, cut), firstFrame) || (cut != std::string::npos && (!whole(text.substr(cut + 1), frameSteps) || frameSteps < 1)))
        {
            std::cerr << "--frames expects FIRST or FIRST:COUNT, whole numbers with COUNT at least 1 (e.g. 0:30)." << std::endl;
            return EXIT_FAILURE;
        }
        if(frameSteps > 1 && (args["--compare"] || args["--compare-methods"] || (args["-g"] && static_cast<int>(args["-g"]) > 1)))
        {
            std::cerr << "--frames with more than one time step cannot be combined with --compare, --compare-methods or -g above 1." << std::endl;
            return EXIT_FAILURE;
        }
    }
    if((args["--frames"] || args["--in-matrix"] || args["--in-range"] || args["--in-chroma"] || args["--in-chroma-site"]) && synthetic)
    {
        std::cerr << "--frames, --in-matrix, --in-range, --in-chroma and --in-chroma-site belong to a light-field video: they need -i with a directory of .y4m files." << std::endl;
        return EXIT_FAILURE;
    }
    int inMatrix = LFI_YUV_BT709, inRange = -1, inChroma = LFI_CHROMA_BILINEAR;
    if(args["--in-matrix"])
    {
        const std::string text = static_cast<std::string>(args["--in-matrix"]);
        if(text != "709" && text != "601")
        {
            std::cerr << "--in-matrix expects 709 or 601." << std::endl;
            return EXIT_FAILURE;
        }
        inMatrix = text == "601" ? LFI_YUV_BT601 : LFI_YUV_BT709;
    }
    if(args["--in-range"])
    {
        const std::string text = static_cast<std::string>(args["--in-range"]);
        if(text != "limited" && text != "full")
        {
            std::cerr << "--in-range expects limited or full." << std::endl;
            return EXIT_FAILURE;
        }
        inRange = text == "full" ? LFI_YUV_FULL : LFI_YUV_LIMITED;
    }
    if(args["--in-chroma"])
    {
        const std::string text = static_cast<std::string>(args["--in-chroma"]);
        if(text != "bilinear" && text != "nearest")
        {
            std::cerr << "--in-chroma expects bilinear or nearest." << std::endl;
            return EXIT_FAILURE;
        }
        inChroma = text == "nearest" ? LFI_CHROMA_NEAREST : LFI_CHROMA_BILINEAR;
    }
    int inChromaSite = lfi::Y4M_SITE_CENTRE;
    if(args["--in-chroma-site"])
    {
        const std::string text = static_cast<std::string>(args["--in-chroma-site"]);
        if(text != "centre" && text != "left" && text != "auto")
        {
            std::cerr << "--in-chroma-site expects centre, left or auto." << std::endl;
            return EXIT_FAILURE;
        }
        inChromaSite = text == "left" ? lfi::Y4M_SITE_LEFT : text == "auto" ? lfi::Y4M_SITE_AUTO : lfi::Y4M_SITE_CENTRE;
    }

    if(args["--compare"] && args["--compare-methods"])
    {
        std::cerr << "--compare (against a directory) and --compare-methods (against the other method) print the same lines: use one of them." << std::endl;
        return EXIT_FAILURE;
    }

    if(args["--compare"] && static_cast<std::string>(args["--compare"]).empty())
    {
        std::cerr << "--compare needs the directory of the images to compare with." << std::endl;
        return EXIT_FAILURE;
    }

    if((args["--compare"] || args["--compare-methods"]) && args["-g"] && static_cast<int>(args["-g"]) > 1)
    {
        std::cerr << "--compare and --compare-methods work on one GPU only (-g 1)." << std::endl;
        return EXIT_FAILURE;
    }

    if(args["-F"] && args["-r"])
    {
        std::cerr << "-F (a focus per view) cannot be combined with -r (all-focus rendering)." << std::endl;
        return EXIT_FAILURE;
    }

    if(args["--view-maps"] && !(args["-c"] && args["-r"]))
    {
        std::cerr << "--view-maps (a focus map per view) needs -c (view-centred shifts) and -r (all-focus rendering)." << std::endl;
        return EXIT_FAILURE;
    }

    try
    {
        int device = static_cast<int>(args["-d"]);
        std::unique_ptr<Interpolator> interpolator;
        if(synthetic)
        {
            std::stringstream spec(static_cast<std::string>(args["--synthetic"]));
            std::string token;
            std::vector<long> numbers;
            while(std::getline(spec, token, ','))
                numbers.push_back(std::stol(token));
            if(numbers.size() < 4)
                throw std::runtime_error("--synthetic expects cols,rows,width,height[,seed]");
            interpolator = std::make_unique<Interpolator>(lfi::IVec2{int(numbers[0]), int(numbers[1])}, lfi::IVec2{int(numbers[2]), int(numbers[3])},
                                                          numbers.size() > 4 ? uint32_t(numbers[4]) : 0x1F1Fu, device);
        }
        else
        {
            Interpolator::setDefaultDevice(device);
            if(args["--mosaic"])
            {
                // "CxR": columns x rows of tiles
                const std::string text = static_cast<std::string>(args["--mosaic"]);
                const size_t cut = text.find_first_of("xX");
                Interpolator::MosaicInput mosaic;
                try
                {
                    if(cut != std::string::npos)
                        mosaic.tiles = {std::stoi(text.substr(0, cut)), std::stoi(text.substr(cut + 1))};
                }
                catch(const std::exception &)
                {
                    mosaic.tiles = {0, 0};
                }
                if(mosaic.tiles.x < 1 || mosaic.tiles.y < 1)
                    throw std::runtime_error("--mosaic expects CxR, columns x rows of tiles, both at least 1");
                mosaic.rowsOrder = mosaicRows;
                mosaic.bottomUp = static_cast<bool>(args["--mosaic-bottom-up"]);
                interpolator = std::make_unique<Interpolator>(path, inChromaSite, mosaic);
            }
            else
                interpolator = std::make_unique<Interpolator>(path, inChromaSite);
        }
        if(args["-n"])
            interpolator->setViewCount(static_cast<int>(args["-n"]));
        if(args["-g"])
            interpolator->setGpuCount(static_cast<int>(args["-g"]));
        if(args["-b"])
            interpolator->setBenchmarkRuns(static_cast<size_t>(static_cast<int>(args["-b"])));
        if(args["--unified-map"])
            interpolator->setUnifiedFocusMap(true);
        if(args["-c"])
            interpolator->setViewCentred(true);
        if(args["--view-maps"])
            interpolator->setViewMaps(true);
        if(args["-F"])
            interpolator->setFocusEnd(static_cast<float>(args["-F"]));
        if(args["--autofocus"])
        {
            std::array<int, 4> region{0, 0, 0, 0}; // all zero: the whole frame
            const std::string text = static_cast<std::string>(args["--autofocus"]);
            if(!text.empty())
            {
                std::stringstream spec(text);
                std::string token;
                size_t count = 0;
                while(std::getline(spec, token, ','))
                {
                    if(count < 4)
                        region[count] = std::stoi(token);
                    count++;
                }
                if(count != 4 || region[0] >= region[2] || region[1] >= region[3])
                    throw std::runtime_error("--autofocus expects x0,y0,x1,y1 with x0 < x1 and y0 < y1");
            }
            interpolator->setAutofocus(region, args["--autofocus-steps"] ? static_cast<int>(args["--autofocus-steps"]) : 32, static_cast<bool>(args["--autofocus-steps"]));
        }
        // a grid of tiles "CxR" (columns x rows)
        const auto tileGrid = [](const std::string &text, const char *flag, const char *meaning = "CxR, columns x rows of tiles, both at least 1") {
            const size_t cut = text.find_first_of("xX");
            lfi::IVec2 grid{0, 0};
            try
            {
                if(cut != std::string::npos)
                    grid = {std::stoi(text.substr(0, cut)), std::stoi(text.substr(cut + 1))};
            }
            catch(const std::exception &)
            {
                grid = {0, 0};
            }
            if(grid.x < 1 || grid.y < 1)
                throw std::runtime_error(std::string(flag) + " expects " + meaning);
            return grid;
        };
        if(args["--map-steps"])
            interpolator->setMapSteps(static_cast<int>(args["--map-steps"]));
        if(args["--tile-steps"])
            interpolator->setTileSteps(static_cast<int>(args["--tile-steps"]));
        if(args["--focus-tiles"])
            interpolator->setFocusTiles(tileGrid(static_cast<std::string>(args["--focus-tiles"]), "--focus-tiles"));
        if(args["--auto-range"])
        {
            const std::string text = static_cast<std::string>(args["--auto-range"]);
            interpolator->setAutoRange(text.empty() ? lfi::IVec2{16, 9} : tileGrid(text, "--auto-range"));
        }
        if(args["-q"])
        {
            std::stringstream spec(static_cast<std::string>(args["-q"]));
            std::string a, b;
            if(!std::getline(spec, a, ',') || !std::getline(spec, b, ','))
                throw std::runtime_error("-q expects cols,rows");
            interpolator->setQuilt({std::stoi(a), std::stoi(b)});
        }
        if(args["--quilt-tile"])
            interpolator->setQuiltTile(tileGrid(static_cast<std::string>(args["--quilt-tile"]), "--quilt-tile", "WxH, the tile's width x height in pixels, both at least 1"));
        if(args["--native"])
        {
            lfi::LensCalibration lens = lensFile.lens;
            if(args["--lens"])
            {
                std::stringstream spec(static_cast<std::string>(args["--lens"]));
                std::string token;
                std::vector<double> numbers;
                try
                {
                    while(std::getline(spec, token, ','))
                        numbers.push_back(std::stod(token));
                }
                catch(const std::exception &)
                {
                    numbers.clear();
                }
                if(numbers.size() < 4 || numbers.size() > 5 || (numbers.size() == 5 && numbers[4] != 0.0 && numbers[4] != 1.0))
                    throw std::runtime_error("--lens expects pitch,slope,center,dpi[,invert] with invert 0 or 1");
                lens.pitch = numbers[0], lens.slope = numbers[1], lens.center = numbers[2], lens.dpi = numbers[3];
                lens.invert = numbers.size() == 5 && numbers[4] == 1.0;
            }
            int views = 0;
            if(args["--native-views"])
            {
                views = static_cast<int>(args["--native-views"]);
                if(views < 1)
                    throw std::runtime_error("--native-views expects the number of views to interlace, at least 1");
            }
            const char *size = "WxH, width x height in pixels, both at least 1";
            const lfi::IVec2 display = tileGrid(static_cast<std::string>(args["--native"]), "--native", size);
            if((lensFile.screenW && lensFile.screenW != display.x) || (lensFile.screenH && lensFile.screenH != display.y))
                std::cout << "Note: the calibration file describes a panel of " << lensFile.screenW << "x" << lensFile.screenH << " pixels, --native asks for "
                          << display.x << "x" << display.y << "." << std::endl;
            interpolator->setNative(display, lens, args["--native-tile"] ? tileGrid(static_cast<std::string>(args["--native-tile"]), "--native-tile", size) : lfi::IVec2{0, 0},
                                    views, nativeFlags);
        }
        if(args["--y4m"])
            interpolator->setY4m(static_cast<std::string>(args["--y4m"]), fpsNum, fpsDen, yuvMatrix, yuvRange);
        if(args["--nv12"])
            interpolator->setNv12(static_cast<std::string>(args["--nv12"]), fpsNum, fpsDen, yuvMatrix, yuvRange);
        if(args["--deep"])
            interpolator->setDeep(true);
        interpolator->setInFrame(inFrameEdges);
        if(inFrameEdges)
            std::cout << "in-frame edges: samples outside their image are left out and the weights of the others renormalised" << std::endl;
        interpolator->setLinearLight(linearLight);
        if(linearLight)
            std::cout << "linear-light blending: samples are decoded from sRGB before the weighted sum and the sum is encoded" << std::endl;
        if(args["--gbrp10"])
            interpolator->setGbrp10(static_cast<std::string>(args["--gbrp10"]));
        if(args["--p010"])
            interpolator->setP010(static_cast<std::string>(args["--p010"]), fpsNum, fpsDen, yuvMatrix, yuvRange);
        interpolator->setYuvDepth(yuvDepth);
        if(args["--quilt-y4m"])
            interpolator->setQuiltY4m(static_cast<std::string>(args["--quilt-y4m"]), fpsNum, fpsDen, yuvMatrix, yuvRange);
        if(args["--rgbd-y4m"])
            interpolator->setRgbdY4m(static_cast<std::string>(args["--rgbd-y4m"]), rgbdView, {rgbdTileW, rgbdTileH}, rgbdMap, static_cast<bool>(args["--rgbd-invert"]), fpsNum,
                                     fpsDen, yuvMatrix, yuvRange);
        interpolator->setChromaSite(outSiting);
        if(args["--compare"])
            interpolator->setCompareDir(static_cast<std::string>(args["--compare"]));
        if(args["--compare-methods"])
            interpolator->setCompareMethods(true);
        if((args["--frames"] || args["--in-matrix"] || args["--in-range"] || args["--in-chroma"] || args["--in-chroma-site"]) && !interpolator->isVideo())
            throw std::runtime_error("--frames, --in-matrix, --in-range, --in-chroma and --in-chroma-site belong to a light-field video: -i has to be a directory of .y4m files, or a .y4m mosaic (--mosaic)");
        if(args["--lean-inputs"])
        {
            if(!interpolator->isVideo())
                throw std::runtime_error("--lean-inputs belongs to a light-field video: -i has to be a directory of .y4m files");
            if(interpolator->inputDepth() == 10)
                throw std::runtime_error("--lean-inputs cannot be combined with 10-bit videos (C420p10): 10-bit frames cannot be expanded straight into the planar copy of the inputs");
            interpolator->setLeanInputs(true);
        }
        if(interpolator->isVideo())
        {
            if(firstFrame + frameSteps > interpolator->frameCount())
                throw std::runtime_error("--frames asks for time steps " + std::to_string(firstFrame) + " to " + std::to_string(firstFrame + frameSteps - 1) +
                                         ", the videos have " + std::to_string(interpolator->frameCount()) + " frames");
            interpolator->setInputYuv(inMatrix, inRange, inChroma);
        }
        for(int step = 0; step < frameSteps; step++)
        {
            std::string stepPath = outputPath;
            if(interpolator->isVideo())
                interpolator->setInputFrame(firstFrame + step);
            if(frameSteps > 1)
            {
                // every time step's files in a directory of its own: <-o>/fTTTT
                const std::string number = std::to_string(firstFrame + step);
                stepPath = outputPath + "/f" + std::string(number.size() < 4 ? 4 - number.size() : 0, '0') + number;
            }
            interpolator->interpolate(stepPath, trajectory, focus, range, method, effect, aspect);
        }
        interpolator->finish();
    }
    catch(const std::exception &e)
    {
        std::cerr << e.what() << std::endl;
        return EXIT_FAILURE;
    }
    return EXIT_SUCCESS;
}
