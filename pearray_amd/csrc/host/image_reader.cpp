// image_reader.cpp -- the image files of (texture ...) blocks: PNG (ISO/IEC 15948) through zlib's inflate, and PFM.
// The reference reads them through OpenImageIO (ImageIO::load); its channel handling is TextureParser.cpp:220-240 (grey is replicated to
// RGB, RGBA keeps RGB) and its linearisation RGBConverter::linearize (spectral/RGBConverter.cpp:53-58).
// Every size is computed in 64 bits and checked before anything is allocated; a malformed file ends in an error code, never a crash
// (tools/fuzz_image.py drives this file under AddressSanitizer).
#include "image_reader.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <zlib.h>

#include "setup.h"

namespace prgpu_host {
namespace {
constexpr uint64_t MAX_FILE_BYTES = uint64_t(1) << 29; // more than the largest image the limits admit can need

int fail(std::string& err, int code, const std::string& msg)
{
	err = msg;
	return code;
}
uint32_t be32(const uint8_t* p) { return (uint32_t(p[0]) << 24) | (uint32_t(p[1]) << 16) | (uint32_t(p[2]) << 8) | uint32_t(p[3]); }

int read_file(const char* path, std::vector<uint8_t>& bytes, std::string& err)
{
	std::FILE* f = std::fopen(path, "rb");
	if (!f)
		return fail(err, PRGPU_EIO, std::string("cannot open image '") + path + "'");
	uint8_t chunk[65536];
	size_t n;
	while ((n = std::fread(chunk, 1, sizeof(chunk), f)) > 0) {
		if (uint64_t(bytes.size()) + n > MAX_FILE_BYTES) {
			std::fclose(f);
			return fail(err, PRGPU_EINVAL, std::string("image '") + path + "' is larger than 512 MiB");
		}
		bytes.insert(bytes.end(), chunk, chunk + n);
	}
	const bool bad = std::ferror(f) != 0;
	std::fclose(f);
	if (bad)
		return fail(err, PRGPU_EIO, std::string("cannot read image '") + path + "'");
	return PRGPU_OK;
}

int check_size(uint64_t w, uint64_t h, std::string& err)
{
	if (w == 0 || h == 0)
		return fail(err, PRGPU_EINVAL, "image is empty");
	if (w > IMAGE_MAX_SIDE || h > IMAGE_MAX_SIDE)
		return fail(err, PRGPU_EINVAL, "image side above 4096");
	return PRGPU_OK;
}

uint8_t paeth(int a, int b, int c)
{
	const int p = a + b - c, pa = std::abs(p - a), pb = std::abs(p - b), pc = std::abs(p - c);
	return uint8_t(pa <= pb && pa <= pc ? a : (pb <= pc ? b : c));
}

int read_png(const std::vector<uint8_t>& file, Image& img, bool header_only, bool scalar, std::string& err)
{
	size_t pos = 8;
	bool have_header = false, have_end = false;
	uint32_t depth = 0, colour = 0;
	std::vector<uint8_t> palette, idat;
	while (!have_end) {
		if (file.size() - pos < 12)
			return fail(err, PRGPU_EIO, "png: file ends inside a chunk (truncated)");
		const uint64_t len = be32(&file[pos]);
		if (len > file.size() - pos - 12)
			return fail(err, PRGPU_EIO, "png: chunk length runs past the end of the file (truncated)");
		const uint8_t* type = &file[pos + 4];
		const uint8_t* data = type + 4;
		if (uint32_t(crc32(0L, type, uInt(len + 4))) != be32(data + len))
			return fail(err, PRGPU_EINVAL, "png: chunk checksum mismatch");
		pos += size_t(len) + 12;
		const bool is_header = std::memcmp(type, "IHDR", 4) == 0;
		if (is_header == have_header)
			return fail(err, PRGPU_EINVAL, "png: IHDR must be the first chunk, once");
		if (is_header) {
			if (len != 13)
				return fail(err, PRGPU_EINVAL, "png: IHDR must hold 13 bytes");
			const uint32_t w = be32(data), h = be32(data + 4);
			if (const int rc = check_size(w, h, err))
				return rc;
			depth  = data[8];
			colour = data[9];
			if (!(colour == 0 || colour == 2 || colour == 3 || colour == 4 || colour == 6))
				return fail(err, PRGPU_EINVAL, "png: unknown colour type");
			if (depth == 1 || depth == 2 || depth == 4)
				return fail(err, PRGPU_EUNSUPPORTED, "png: bit depths below 8 are not supported");
			if (!(depth == 8 || depth == 16) || (colour == 3 && depth != 8))
				return fail(err, PRGPU_EINVAL, "png: invalid bit depth");
			if (data[10] != 0 || data[11] != 0)
				return fail(err, PRGPU_EINVAL, "png: unknown compression or filter method");
			if (data[12] == 1)
				return fail(err, PRGPU_EUNSUPPORTED, "png: interlaced files are not supported");
			if (data[12] != 0)
				return fail(err, PRGPU_EINVAL, "png: unknown interlace method");
			img.width			 = w;
			img.height			 = h;
			img.channels_in_file = colour == 0 ? 1 : colour == 4 ? 2 : colour == 6 ? 4 : 3;
			img.linearised		 = true;
			have_header			 = true;
			if (header_only)
				return PRGPU_OK;
		} else if (std::memcmp(type, "PLTE", 4) == 0) {
			if (len == 0 || len % 3 != 0 || len > 768 || !palette.empty())
				return fail(err, PRGPU_EINVAL, "png: malformed palette");
			palette.assign(data, data + len);
		} else if (std::memcmp(type, "IDAT", 4) == 0) {
			if (uint64_t(idat.size()) + len > MAX_FILE_BYTES)
				return fail(err, PRGPU_EINVAL, "png: image data too large");
			idat.insert(idat.end(), data, data + len);
		} else if (std::memcmp(type, "IEND", 4) == 0) {
			have_end = true;
		} // tRNS and every other ancillary chunk: dropped
	}
	if (colour == 3 && palette.empty())
		return fail(err, PRGPU_EINVAL, "png: palette image without a palette");
	if (idat.empty())
		return fail(err, PRGPU_EINVAL, "png: no image data");
	const uint32_t samples = colour == 3 ? 1u : img.channels_in_file;
	const uint64_t bpp	   = uint64_t(samples) * (depth / 8);						// bytes per pixel: at most 8
	const uint64_t stride  = uint64_t(img.width) * bpp;								// at most 32 KiB
	const uint64_t raw_len = uint64_t(img.height) * (stride + 1);					// at most 128 MiB + 4 KiB
	std::vector<uint8_t> raw(size_t(raw_len) + 1);									// one spare byte: a stream that holds more is noticed
	z_stream zs;
	std::memset(&zs, 0, sizeof(zs));
	if (inflateInit(&zs) != Z_OK)
		return fail(err, PRGPU_EINVAL, "png: inflate could not start");
	zs.next_in		 = idat.data();
	zs.avail_in		 = uInt(idat.size());
	zs.next_out		 = raw.data();
	zs.avail_out	 = uInt(raw.size());
	const int zrc	 = inflate(&zs, Z_FINISH);
	const uint64_t n = zs.total_out;
	inflateEnd(&zs);
	if (zrc != Z_STREAM_END || n != raw_len)
		return fail(err, PRGPU_EINVAL, "png: the compressed stream is damaged or does not hold height x (1 + row) bytes");
	// the five row filters, in place; `prev` is the row above after reconstruction (absent for the first row: zeros)
	for (uint64_t y = 0; y < img.height; ++y) {
		uint8_t* row		= &raw[size_t(y * (stride + 1))];
		const uint8_t ft	= row[0];
		uint8_t* cur		= row + 1;
		const uint8_t* prev = y ? cur - (stride + 1) : nullptr;
		if (ft > 4)
			return fail(err, PRGPU_EINVAL, "png: unknown row filter");
		for (uint64_t i = 0; i < stride; ++i) {
			const int a = i >= bpp ? cur[i - bpp] : 0, b = prev ? prev[i] : 0, c = (prev && i >= bpp) ? prev[i - bpp] : 0;
			const int add = ft == 0 ? 0 : ft == 1 ? a : ft == 2 ? b : ft == 3 ? ((a + b) >> 1) : paeth(a, b, c);
			cur[i]		  = uint8_t(cur[i] + add);
		}
	}
	img.rgb.resize(size_t(uint64_t(img.width) * img.height * (scalar ? 1u : 3u)));
	const float scale = depth == 8 ? 255.0f : 65535.0f;
	for (uint64_t y = 0; y < img.height; ++y) {
		const uint8_t* cur = &raw[size_t(y * (stride + 1)) + 1];
		for (uint64_t x = 0; x < img.width; ++x) {
			const uint8_t* px = cur + x * bpp;
			if (scalar) { // the file's first channel as it is (a palette image: the entry's red), no linearisation
				float& value = img.rgb[size_t(y * img.width + x)];
				if (colour == 3) {
					if (size_t(px[0]) * 3 + 2 >= palette.size())
						return fail(err, PRGPU_EINVAL, "png: palette index out of range");
					value = palette[size_t(px[0]) * 3] / 255.0f;
				} else {
					value = float(depth == 8 ? uint32_t(px[0]) : ((uint32_t(px[0]) << 8) | px[1])) / scale;
				}
				continue;
			}
			float* out		  = &img.rgb[size_t(y * img.width + x) * 3];
			if (colour == 3) {
				if (size_t(px[0]) * 3 + 2 >= palette.size())
					return fail(err, PRGPU_EINVAL, "png: palette index out of range");
				for (int k = 0; k < 3; ++k)
					out[k] = image_linearise(palette[size_t(px[0]) * 3 + k] / 255.0f);
				continue;
			}
			for (int k = 0; k < 3; ++k) {
				const uint32_t s  = samples >= 3 ? uint32_t(k) : 0u; // grey (+ alpha): replicated; RGBA: alpha dropped
				const uint8_t* sp = px + s * (depth / 8);
				const uint32_t v  = depth == 8 ? sp[0] : ((uint32_t(sp[0]) << 8) | sp[1]);
				out[k]			  = image_linearise(float(v) / scale);
			}
		}
	}
	return PRGPU_OK;
}

// one whitespace-delimited header token of a PFM, starting at `pos`; leaves `pos` on the whitespace byte that ends it
bool pfm_token(const std::vector<uint8_t>& file, size_t& pos, std::string& tok)
{
	auto space = [](uint8_t c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r'; };
	while (pos < file.size() && space(file[pos]))
		++pos;
	tok.clear();
	while (pos < file.size() && !space(file[pos]) && tok.size() < 32)
		tok.push_back(char(file[pos++]));
	return !tok.empty() && pos < file.size() && space(file[pos]);
}

int read_pfm(const std::vector<uint8_t>& file, Image& img, bool header_only, bool scalar, std::string& err)
{
	size_t pos = 0;
	std::string magic, ws, hs, ss;
	if (!pfm_token(file, pos, magic) || !pfm_token(file, pos, ws) || !pfm_token(file, pos, hs) || !pfm_token(file, pos, ss))
		return fail(err, PRGPU_EIO, "pfm: file ends inside the header (truncated)");
	++pos; // the single whitespace byte after the scale
	char* end			 = nullptr;
	const uint64_t w	 = std::strtoull(ws.c_str(), &end, 10);
	const bool w_ok		 = end && *end == 0 && ws[0] >= '0' && ws[0] <= '9';
	const uint64_t h	 = std::strtoull(hs.c_str(), &end, 10);
	const bool h_ok		 = end && *end == 0 && hs[0] >= '0' && hs[0] <= '9';
	const double scale	 = std::strtod(ss.c_str(), &end);
	const bool s_ok		 = end && *end == 0 && std::isfinite(scale) && scale != 0.0;
	if (!w_ok || !h_ok || !s_ok)
		return fail(err, PRGPU_EINVAL, "pfm: malformed header (width, height, non-zero scale)");
	if (const int rc = check_size(w, h, err))
		return rc;
	const uint32_t ch	 = magic == "PF" ? 3u : 1u;
	img.width			 = uint32_t(w);
	img.height			 = uint32_t(h);
	img.channels_in_file = ch;
	img.linearised		 = false;
	if (header_only)
		return PRGPU_OK;
	const uint64_t need = w * h * ch * 4; // at most 192 MiB
	if (need > file.size() - pos)
		return fail(err, PRGPU_EIO, "pfm: file ends inside the pixel data (truncated)");
	const bool little = scale < 0.0;
	const uint32_t out_ch = scalar ? 1u : 3u; // scalar: the file's first channel alone
	img.rgb.resize(size_t(w * h * out_ch));
	for (uint64_t y = 0; y < h; ++y) { // the file's rows run bottom-up
		const uint8_t* row = &file[pos + size_t((h - 1 - y) * w * ch * 4)];
		for (uint64_t x = 0; x < w; ++x)
			for (uint32_t k = 0; k < out_ch; ++k) {
				const uint8_t* b = row + (x * ch + (ch == 3 ? k : 0u)) * 4;
				const uint32_t u = little ? (uint32_t(b[0]) | (uint32_t(b[1]) << 8) | (uint32_t(b[2]) << 16) | (uint32_t(b[3]) << 24)) : be32(b);
				float v;
				std::memcpy(&v, &u, 4);
				if (!std::isfinite(v))
					return fail(err, PRGPU_EINVAL, "pfm: a sample is not finite");
				img.rgb[size_t(y * w + x) * out_ch + k] = v;
			}
	}
	return PRGPU_OK;
}
} // namespace

float image_linearise(float x) { return (x <= 0.04045f) ? x / 12.92f * x : std::pow((x + 0.055f) / 1.055f, 2.4f); }

int read_image(const char* path, Image& img, bool header_only, std::string& err, bool scalar)
{
	img = Image();
	std::vector<uint8_t> file;
	if (const int rc = read_file(path, file, err))
		return rc;
	static const uint8_t png_magic[8] = { 0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A };
	int rc;
	if (file.size() >= 8 && std::memcmp(file.data(), png_magic, 8) == 0)
		rc = read_png(file, img, header_only, scalar, err);
	else if (file.size() >= 3 && file[0] == 'P' && (file[1] == 'F' || file[1] == 'f') && (file[2] == '\n' || file[2] == ' ' || file[2] == '\r' || file[2] == '\t'))
		rc = read_pfm(file, img, header_only, scalar, err);
	else if (file.size() < 8)
		rc = fail(err, PRGPU_EIO, "image file is shorter than a signature (truncated)");
	else
		rc = fail(err, PRGPU_EUNSUPPORTED, "image is neither a PNG nor a PFM file");
	if (scalar)
		img.linearised = false;
	if (rc != PRGPU_OK) {
		err = std::string("image '") + path + "': " + err;
		img = Image();
	}
	return rc;
}
} // namespace prgpu_host

extern "C" int prgpu_image_load(const char* path, uint32_t* width, uint32_t* height, uint32_t* channels_in_file, int* linearised, float* rgb)
{
	using namespace prgpu_host;
	if (!path || !width || !height)
		return set_last_error(PRGPU_EINVAL, "prgpu_image_load: null argument");
	Image img;
	std::string err;
	const int rc = read_image(path, img, rgb == nullptr, err);
	if (rc != PRGPU_OK)
		return set_last_error(rc, "prgpu_image_load: " + err);
	*width	= img.width;
	*height = img.height;
	if (channels_in_file)
		*channels_in_file = img.channels_in_file;
	if (linearised)
		*linearised = img.linearised ? 1 : 0;
	if (rgb)
		std::memcpy(rgb, img.rgb.data(), img.rgb.size() * sizeof(float));
	return PRGPU_OK;
}

extern "C" int prgpu_image_load_scalar(const char* path, uint32_t* width, uint32_t* height, uint32_t* channels_in_file, float* values)
{
	using namespace prgpu_host;
	if (!path || !width || !height)
		return set_last_error(PRGPU_EINVAL, "prgpu_image_load_scalar: null argument");
	Image img;
	std::string err;
	const int rc = read_image(path, img, values == nullptr, err, true);
	if (rc != PRGPU_OK)
		return set_last_error(rc, "prgpu_image_load_scalar: " + err);
	*width	= img.width;
	*height = img.height;
	if (channels_in_file)
		*channels_in_file = img.channels_in_file;
	if (values)
		std::memcpy(values, img.rgb.data(), img.rgb.size() * sizeof(float));
	return PRGPU_OK;
}
