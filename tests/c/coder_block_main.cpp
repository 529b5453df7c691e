// The replay rule of jpeg2png_amd/csrc/j2p_coder_block.h, driven without a device (tests/test_coder_block_cpu.py): `memory` is
// a host buffer that is REPLACED — the old one freed, the new one filled with a poison byte — whenever a request exceeds it, as
// the pool and a solver's scratch replace a device block.  A stage appends its name to a log and writes 16 bytes into the block;
// the second and the third read what the stage before them wrote, as the coders' stages do.  Prints "ok", or what failed.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "j2p_coder_block.h"

#define CHECK(cond)                                                              \
        do {                                                                     \
                if(!(cond)) {                                                    \
                        printf("line %d: %s (log \"%s\")\n", __LINE__, #cond, log.c_str()); \
                        return 1;                                                \
                }                                                                \
        } while(0)

namespace {

constexpr unsigned char kPoison = 0xee;
constexpr int kRefused = -3;

struct FakeMemory {
        unsigned char *buffer = nullptr;
        size_t bytes = 0;
        unsigned calls = 0;
        bool refuse = false;
        ~FakeMemory() { free(buffer); }
        int operator()(size_t want, void **p, bool *moved)
        {
                calls++;
                if(refuse) { return kRefused; }
                *moved = bytes < want;
                if(*moved) {
                        free(buffer);
                        buffer = static_cast<unsigned char *>(malloc(want));
                        if(!buffer) { return -2; }
                        memset(buffer, kPoison, want);
                        bytes = want;
                }
                *p = buffer;
                return 0;
        }
};

// region k of the block holds 16 bytes of 'c' + k, and everything behind the regions written so far is poison
bool holds(const j2p_coder_block &block, unsigned regions, size_t bytes)
{
        for(size_t i = 0; i < bytes; i++) {
                const unsigned char want = i < 16 * regions ? (unsigned char)('c' + i / 16) : kPoison;
                if(*block.at<unsigned char>(i) != want) { return false; }
        }
        return true;
}

}  // namespace

int main()
{
        std::string log;
        FakeMemory fake;
        j2p_coder_block block([&](size_t bytes, void **p, bool *moved) { return fake(bytes, p, moved); });
        const auto c = [&] {
                log += "c,";
                memset(block.at(0), 'c', 16);
        };
        const auto l = [&] {
                log += "l,";
                for(int i = 0; i < 16; i++) { *block.at<unsigned char>(16 + i) = (unsigned char)(*block.at<unsigned char>(i) + 1); }
        };
        const auto p = [&] {
                log += "p,";
                for(int i = 0; i < 16; i++) { *block.at<unsigned char>(32 + i) = (unsigned char)(*block.at<unsigned char>(16 + i) + 1); }
        };
        // the first request runs nothing; a stage runs at once and exactly once
        CHECK(block.grow(64) == 0 && log.empty() && fake.calls == 1 && block.at(0) == (char *)fake.buffer);
        CHECK(holds(block, 0, 64));
        block.stage(c);
        CHECK(log == "c," && holds(block, 1, 64));
        // a request that fits runs nothing and keeps the base
        const char *const before = block.at(0);
        CHECK(block.grow(64) == 0 && block.grow(17) == 0 && log == "c," && block.at(0) == before && fake.calls == 3);
        block.stage(l);
        CHECK(log == "c,l," && holds(block, 2, 64));
        // an error of memory comes back as it is, runs no stage and leaves the base
        fake.refuse = true;
        CHECK(block.grow(1 << 20) == kRefused && log == "c,l," && block.at(0) == before && block.at<int>(8) == (int *)(before + 8));
        fake.refuse = false;
        // a request that moves the block runs the stages so far, in their order, in the new block — and not the one that follows
        log += "|";
        CHECK(block.grow(100) == 0 && log == "c,l,|c,l," && block.at(0) == (char *)fake.buffer && holds(block, 2, 100));
        block.stage(p);
        CHECK(log == "c,l,|c,l,p," && holds(block, 3, 100));
        log += "|";
        CHECK(block.grow(101) == 0 && log == "c,l,|c,l,p,|c,l,p," && block.at(0) == (char *)fake.buffer && holds(block, 3, 101));
        // ... and a smaller request afterwards none
        CHECK(block.grow(48) == 0 && log == "c,l,|c,l,p,|c,l,p," && holds(block, 3, 101));
        printf("ok\n");
        return 0;
}
