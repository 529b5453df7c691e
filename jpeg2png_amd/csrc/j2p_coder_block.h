// jpeg2png_amd — the one block of device memory a file coder works in (j2p_codec.hip: j2p_encode_scan, j2p_encode_progressive,
// j2p_png_write), whose final size is not known when the call starts.  The coder asks for it again whenever it knows more (grow),
// the earlier times with a guess for the rest; `memory` (j2p_internal.h) answers with the same block while that is large enough and
// with ANOTHER one, the contents lost, once it is not.  What the coder has queued into the block by then is registered here as
// stages, and a block that moved has every one of them queued again, in their order, before grow returns: what is queued again is
// by construction what was queued.  What the coder has brought down to the host meanwhile (counts, tables, sizes) is no stage.
// Host code only, and no HIP: tests/c/coder_block_main.cpp drives it with host memory.
#pragma once
#include <assert.h>
#include <stddef.h>

#include <functional>

class j2p_coder_block {
public:
        explicit j2p_coder_block(std::function<int(size_t, void **, bool *)> memory) : memory_(std::move(memory)) {}

        // the block with at least `bytes` bytes.  memory's error (not 0) comes back as it is: nothing is queued, the base stays
        int grow(size_t bytes)
        {
                void *p = nullptr;
                bool moved = false;
                if(const int rc = memory_(bytes, &p, &moved); rc != 0) { return rc; }
                base_ = static_cast<char *>(p);
                for(unsigned k = 0; moved && k < nstages_; k++) { stages_[k].run(stages_[k].queue); }
                return 0;
        }
        // queue() now, and again after every move from here on.  It finds the block through at(), each time it runs; the block
        // keeps a pointer to it, not a copy, so it is a named closure of the coder's that lives as long as the block is used
        template<class F> void stage(F &queue)
        {
                assert(nstages_ < kStages);
                stages_[nstages_++] = {[](void *f) { (*static_cast<F *>(f))(); }, const_cast<void *>(static_cast<const void *>(&queue))};
                queue();
        }
        // the part at `offset` of the block as it is now
        template<class T = char> T *at(size_t offset) const { return reinterpret_cast<T *>(base_ + offset); }

private:
        static constexpr unsigned kStages = 3;  // the most a coder has: coefficients, lengths, streams
        struct Stage {
                void (*run)(void *);
                void *queue;
        };
        const std::function<int(size_t, void **, bool *)> memory_;
        char *base_ = nullptr;
        Stage stages_[kStages] = {};
        unsigned nstages_ = 0;
};
