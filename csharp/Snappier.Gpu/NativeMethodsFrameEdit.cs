// P/Invoke surface of libsnappier_hip_frame_edit.so -- one declaration per function of include/snappier_hip_frame_edit.h, same order.
// That library is linked against libsnappier_hip.so and takes its contexts (NativeMethods.snp_ctx_create).
using System;
using System.Runtime.InteropServices;

namespace Snappier.Gpu;

internal static unsafe class NativeMethodsFrameEdit
{
    private const string Lib = "snappier_hip_frame_edit";                       // libsnappier_hip_frame_edit.so
    private const CallingConvention Cc = CallingConvention.Cdecl;

    // ---- batch, device pointers (asynchronous on the context's stream): a sorted edit script per framed stream kept with its index (dEdFirst: nstreams + 1, CSR over the nedits edits), out of place
    // (the five dIdx* pointers are the arrays NativeMethodsFrameIndex.snp_frame_read_indexed_batch takes, the five dNew* the index of the new streams; dEdStatus holds nedits verdicts; dOutBound may be IntPtr.Zero)
    [DllImport(Lib, CallingConvention = Cc)] internal static extern ulong snp_frame_edit_indexed_workspace(uint nstreams, uint nedits, uint maxSlots, ulong stageCap, uint chunkBytes);
    [DllImport(Lib, CallingConvention = Cc)] internal static extern SnpStatus snp_frame_edit_indexed_batch(IntPtr ctx, IntPtr dIn, IntPtr dInOff, IntPtr dInLen, uint nstreams, IntPtr dIdxFirst, IntPtr dIdxStart, IntPtr dIdxPos, IntPtr dIdxTotal, IntPtr dIdxTail, ulong nentries, IntPtr dSrc, IntPtr dEdFirst, IntPtr dEdOff, IntPtr dEdDel, IntPtr dEdIns, IntPtr dSrcOff, uint nedits, uint chunkBytes, uint maxSlots, ulong stageCap, IntPtr dOut, IntPtr dOutOff, IntPtr dOutCap, IntPtr dOutLen, IntPtr dStatus, IntPtr dEdStatus, IntPtr dNewFirst, IntPtr dNewStart, IntPtr dNewPos, IntPtr dNewTotal, IntPtr dNewTail, IntPtr dOutBound, IntPtr dWork, IntPtr dResult);
}
