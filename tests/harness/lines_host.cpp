// lines_host.cpp — every worker prints lines to std::cout in several pieces,
// all workers at once, the way the reference's harnesses print their result
// (`cout << "got error value: " << a << ", " << b << '\n'`).  With the nodes
// as threads of one process the lines have to come out whole.  Run by
// tests/test_host_lines.py; needs no GPU.
#include <cstdlib>
#include <iostream>

#include "ps/ps.h"

using namespace ps;

int main(int argc, char* argv[]) {
  Start(0, argc, argv);
  const int lines = std::atoi(argv[argc - 1]);  // the last argument: lines per worker
  if (IsWorker()) {
    const int rank = MyRank();
    Barrier(0, kWorkerGroup);  // every worker starts printing together
    for (int i = 0; i < lines; ++i) std::cout << "worker " << rank << ", line " << i << ": " << 0 << ", " << 0 << '\n';
    Barrier(0, kWorkerGroup);  // the unfinished lines come after every whole one
    std::cout << "worker " << rank << " left without a newline";
  }
  Finalize(0, true);
  return 0;
}
