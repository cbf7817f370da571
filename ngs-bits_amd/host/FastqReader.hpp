// The text of a FASTQ file for ReadQC: gzip (any number of members, so BGZF as well) or plain text, through zlib, in pieces of the caller's size. What
// FastqFileStream gets from VersatileFile / gzread (src/cppNGS/FastqFileStream.cpp:112-131); inflation stays on the host.
#pragma once
#include "core.hpp"
#include <zlib.h>
#include <cstring>

namespace ngsbits {

class FastqTextReader
{
public:
	explicit FastqTextReader(const std::string& path) : path_(path), in_(1 << 20)
	{
		f_ = fopen(path.c_str(), "rb");
		if (!f_) NB_THROW(FileAccessException, "Could not open file '" + path + "' for reading!");
		fill();
		gzip_ = have_ >= 2 && in_[0] == 0x1f && in_[1] == 0x8b;
		if (gzip_)
		{
			memset(&zs_, 0, sizeof(zs_));
			if (inflateInit2(&zs_, 15 + 16) != Z_OK) NB_THROW(ProgrammingException, "inflateInit2 failed");
			zinit_ = true;
		}
	}
	~FastqTextReader() { if (zinit_) inflateEnd(&zs_); if (f_) fclose(f_); }
	FastqTextReader(const FastqTextReader&) = delete; FastqTextReader& operator=(const FastqTextReader&) = delete;

	// up to cap bytes of text; fewer only at the end of the file, 0: the end
	size_t read(uint8_t* out, size_t cap)
	{
		size_t got = 0;
		while (got < cap && !done_)
		{
			if (pos_ == have_) { fill(); if (have_ == 0) { if (gzip_ && in_member_) NB_THROW(FileParseException, "Unexpected end of gzip stream in file '" + path_ + "'!"); done_ = true; break; } }
			if (!gzip_)
			{
				const size_t k = std::min(cap - got, have_ - pos_);
				memcpy(out + got, in_.data() + pos_, k); pos_ += k; got += k;
				continue;
			}
			if (!in_member_)
			{
				// between members: another one starts with the gzip magic; anything else behind the last member is ignored, as gzread ignores it
				if (have_ - pos_ < 2) { refill_keep(); if (have_ - pos_ < 2) { done_ = true; break; } }
				if (in_[pos_] != 0x1f || in_[pos_ + 1] != 0x8b) { done_ = true; break; }
				in_member_ = true;
			}
			zs_.next_in = in_.data() + pos_; zs_.avail_in = (uInt)(have_ - pos_);
			zs_.next_out = out + got; zs_.avail_out = (uInt)std::min<size_t>(cap - got, 1u << 30);
			const int rc = inflate(&zs_, Z_NO_FLUSH);
			pos_ = have_ - zs_.avail_in; got = (size_t)(zs_.next_out - out);
			if (rc == Z_STREAM_END) { in_member_ = false; inflateReset(&zs_); }
			else if (rc != Z_OK && rc != Z_BUF_ERROR) NB_THROW(FileParseException, "Error while decompressing file '" + path_ + "': " + (zs_.msg ? zs_.msg : "zlib error " + std::to_string(rc)));
		}
		return got;
	}
private:
	void fill() { have_ = fread(in_.data(), 1, in_.size(), f_); pos_ = 0; }
	void refill_keep() { const size_t k = have_ - pos_; memmove(in_.data(), in_.data() + pos_, k); have_ = k + fread(in_.data() + k, 1, in_.size() - k, f_); pos_ = 0; }
	std::string path_; FILE* f_ = nullptr; std::vector<uint8_t> in_; size_t have_ = 0, pos_ = 0;
	bool gzip_ = false, zinit_ = false, in_member_ = false, done_ = false; z_stream zs_;
};

} // namespace ngsbits
