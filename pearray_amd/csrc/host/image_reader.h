// image_reader.h -- reads the image files a (texture ...) block names: PNG (through zlib's inflate) and PFM.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace prgpu_host {
constexpr uint32_t IMAGE_MAX_SIDE = 4096; // a wider or taller image is refused

struct Image {
	uint32_t width = 0, height = 0;
	uint32_t channels_in_file = 0; // 1 grey, 2 grey + alpha, 3 RGB, 4 RGBA (a palette counts as RGB)
	bool linearised			  = false; // PNG: the samples went through RGBConverter::linearize; PFM is taken as linear
	std::vector<float> rgb;			   // height x width x 3, rows top-down (scalar mode: height x width x 1)
};

// PNG samples -> linear, as RGBConverter::linearize (spectral/RGBConverter.cpp:53-58) writes it: the toe is x / 12.92 * x, a quirk kept
float image_linearise(float x);
// PRGPU_OK, or PRGPU_EIO / PRGPU_EINVAL / PRGPU_EUNSUPPORTED with `err` set.  header_only: width, height and channels_in_file only.
// scalar: what a `(texture :type 'scalar')` block reads (ScalarImageNode, shader/ImageNode.cpp:183-241): the file's FIRST channel alone, one
// float per pixel, the raw value (a PNG integer / 255 or 65535, a PFM float as it is) -- no linearisation
int read_image(const char* path, Image& img, bool header_only, std::string& err, bool scalar = false);
} // namespace prgpu_host
